"""fhe_gpu -- Python host mirror of the reference operator interface over the
MI355X C-ABI (``include/fhe_gpu.h``, ``build/libfhe_gpu.so``).

Class and method names follow the reference C++ classes so parity tests read
like the reference's own tests:

=============================  ==============================================
reference (cpp/include/...)    here
=============================  ==============================================
NTTProcessor                   :class:`NTTProcessor`   (ntt_processor.h:49-306)
PolynomialRing                 :class:`PolynomialRing` (polynomial_ring.h:101-516)
PolynomialRing(degree, moduli) :class:`RNSPolynomialRing` (polynomial_ring.cpp:224-237)
ModularArithmetic              :class:`ModularArithmetic` (modular_arithmetic.h:20-80;
                               the N-API class of index.d.ts:32-44)
BarrettReducer                 :class:`BarrettReducer` (modular_arithmetic.h:82-)
MultiLimbModularArithmetic     :class:`MultiLimbModularArithmetic`
BootstrapEngine::external_product  :class:`ExternalProduct`
BootstrapEngine (cmux, blind_rotate, :class:`BootstrapEngine`
  sample_extract, key_switch, ...)
EncryptionEngine::multiply /   :class:`EncryptionEngine`, :class:`EvaluationKey`
  relinearize / multiply_relin
HardwareDetector::detect       :func:`detect_hardware`
=============================  ==============================================

Buffers: numpy ``uint64`` arrays (host; the call stages through HBM) or torch
CUDA tensors of dtype int64/uint64 (device-resident; enqueued on the current
torch stream, no host sync).  Shapes are ``[..., n]``: leading dims are the
batch.  Errors raise :class:`FHEError` carrying the reference's exception text.

There is no CPU fallback: if the HIP library is missing or no GPU is present
every compute call raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Optional

import numpy as np

try:  # share torch's HIP runtime when torch is present (one runtime per process)
    import torch  # noqa: F401

    _HAVE_TORCH = True
except Exception:  # pragma: no cover
    torch = None
    _HAVE_TORCH = False

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
LIB_PATH = os.environ.get("FHE_GPU_LIB", os.path.join(_ROOT, "build", "libfhe_gpu.so"))

FHE_OK = 0
FHE_HOST, FHE_DEVICE = 0, 1
MODE_COMPAT, MODE_NEGACYCLIC = 0, 1

ERROR_NAMES = {
    -1: "DEGREE_POW2", -2: "DEGREE_RANGE", -3: "MODULUS_EVEN", -4: "NOT_NTT_FRIENDLY",
    -5: "COUNT", -6: "NO_ROOT", -7: "MONT_MODULUS", -8: "ZERO_MODULUS", -9: "INVALID_ARG",
    -10: "UNSUPPORTED", -11: "DEVICE", -12: "OOM",
}


class FHEError(ValueError):
    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code
        self.name = ERROR_NAMES.get(code, "UNKNOWN")


class HwCaps(C.Structure):
    _fields_ = [
        ("device_count", C.c_int32), ("compute_units", C.c_int32), ("wavefront_size", C.c_int32),
        ("xcds", C.c_int32), ("hbm_bytes", C.c_uint64), ("lds_bytes_per_cu", C.c_uint64),
        ("arch", C.c_char * 32), ("name", C.c_char * 96),
    ]


class CtxInfo(C.Structure):
    _fields_ = [
        ("n", C.c_uint32), ("log_n", C.c_uint32), ("q", C.c_uint64), ("psi", C.c_uint64),
        ("psi_inv", C.c_uint64), ("inv_n", C.c_uint64), ("mode", C.c_int32), ("word_bits", C.c_int32),
        ("device", C.c_int32), ("polys_per_block", C.c_int32), ("threads_per_block", C.c_int32),
    ]


class ScaleInfo(C.Structure):
    _fields_ = [
        ("q", C.c_uint64), ("t", C.c_uint64), ("aux", C.c_uint64 * 2), ("n", C.c_uint32), ("naux", C.c_uint32),
        ("max_count", C.c_uint64),
    ]


class SimdInfo(C.Structure):
    _fields_ = [
        ("q", C.c_uint64), ("t", C.c_uint64), ("psi", C.c_uint64), ("n", C.c_uint32), ("word_bits", C.c_int32),
    ]


u64p = C.POINTER(C.c_uint64)
vp = C.c_void_p

# (name, restype, argtypes) of every entry point declared in include/fhe_gpu.h
SIGNATURES = [
    ("fhe_last_error", C.c_char_p, []),
    ("fhe_version", C.c_char_p, []),
    ("fhe_build_id", C.c_char_p, []),
    ("fhe_detect", C.c_int, [C.POINTER(HwCaps)]),
    ("fhe_ctx_create", C.c_int, [C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.POINTER(vp)]),
    ("fhe_ctx_destroy", None, [vp]),
    ("fhe_ctx_create_multi", C.c_int, [C.c_uint32, C.c_uint64, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]),
    ("fhe_ctx_device_count", C.c_int, [vp, C.POINTER(C.c_int)]),
    ("fhe_ctx_sub", C.c_int, [vp, C.c_int, C.POINTER(vp)]),
    ("fhe_ctx_set_stream", C.c_int, [vp, vp]),
    ("fhe_ctx_stream", vp, [vp]),
    ("fhe_ctx_synchronize", C.c_int, [vp]),
    ("fhe_ctx_get_info", C.c_int, [vp, C.POINTER(CtxInfo)]),
    ("fhe_ctx_get_twiddles", C.c_int, [vp, vp, vp]),
    ("fhe_ntt_fwd_batch", C.c_int, [vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_ntt_inv_batch", C.c_int, [vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_ntt_fwd_mul_batch", C.c_int, [vp, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_polymul_batch", C.c_int, [vp, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_pointwise_batch", C.c_int, [vp, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_poly_add_batch", C.c_int, [vp, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_poly_sub_batch", C.c_int, [vp, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_poly_neg_batch", C.c_int, [vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_poly_mul_scalar_batch", C.c_int, [vp, vp, C.c_uint64, vp, C.c_size_t, C.c_int]),
    ("fhe_ct_sum_batch", C.c_int, [vp, vp, C.c_uint32, C.c_size_t, C.c_size_t, C.c_int, vp, C.c_int]),
    ("fhe_ct_sum_ptrs", C.c_int, [vp, vp, C.c_uint32, C.c_size_t, C.c_int, vp]),
    ("fhe_ct_dot_batch", C.c_int, [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, vp, C.c_int]),
    ("fhe_ct_dot_ptrs", C.c_int, [vp, vp, vp, C.c_size_t, C.c_int, C.c_int, vp]),
    ("fhe_ct_sum_scaled_batch", C.c_int, [vp, vp, vp, C.c_uint32, C.c_size_t, C.c_size_t, C.c_int, vp, C.c_int]),
    ("fhe_ct_sum_scaled_ptrs", C.c_int, [vp, vp, vp, C.c_uint32, C.c_size_t, C.c_int, vp]),
    ("fhe_ct_dot_plain_batch", C.c_int, [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, vp, C.c_int]),
    ("fhe_ct_dot_plain_ptrs", C.c_int, [vp, vp, vp, C.c_size_t, C.c_int, C.c_int, vp]),
    ("fhe_ggsw_prepare", C.c_int, [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_int]),
    ("fhe_external_product_batch", C.c_int,
     [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_decompose_batch", C.c_int, [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_rns_ctx_create", C.c_int, [C.c_uint32, u64p, C.c_uint32, C.c_int, C.c_int, C.POINTER(vp)]),
    ("fhe_rns_ctx_destroy", None, [vp]),
    ("fhe_rns_ctx_limb", C.c_int, [vp, C.c_uint32, C.POINTER(vp)]),
    ("fhe_rns_ntt_fwd_batch", C.c_int, [vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_rns_ntt_inv_batch", C.c_int, [vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_rns_polymul_batch", C.c_int, [vp, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_rns_pointwise_batch", C.c_int, [vp, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_rns_add_batch", C.c_int, [vp, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_rns_sub_batch", C.c_int, [vp, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_ct_multiply_batch", C.c_int, [vp, vp, vp, vp, C.c_size_t, C.c_int, C.c_int]),
    ("fhe_relin_key_prepare", C.c_int, [vp, C.c_uint32, vp, vp, C.c_int]),
    ("fhe_relinearize_batch", C.c_int, [vp, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_ct_multiply_relin_batch", C.c_int,
     [vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_poly_galois_batch", C.c_int, [vp, C.c_uint32, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_switch_key_generate", C.c_int,
     [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, u64p, C.c_uint64, C.c_double, vp, C.c_int]),
    ("fhe_ct_galois_batch", C.c_int,
     [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_int, vp, C.c_size_t, C.c_int]),
    ("fhe_ct_trace_batch", C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_ct_square_batch", C.c_int, [vp, vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int]),
    ("fhe_ct_square_relin_batch", C.c_int,
     [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_size_t, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_scale_ctx_create", C.c_int, [vp, C.c_uint64, C.POINTER(vp)]),
    ("fhe_scale_ctx_destroy", None, [vp]),
    ("fhe_scale_ctx_get_info", C.c_int, [vp, C.POINTER(ScaleInfo)]),
    ("fhe_poly_center_lift_batch", C.c_int, [vp, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_ct_center_lift_batch", C.c_int, [vp, vp, vp, C.c_size_t, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_poly_scale_round_batch", C.c_int, [vp, vp, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_ct_multiply_scaled_batch", C.c_int, [vp, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_ct_dot_scaled_batch", C.c_int, [vp, vp, vp, C.c_size_t, C.c_size_t, vp, C.c_int]),
    ("fhe_ct_square_scaled_batch", C.c_int, [vp, vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int]),
    ("fhe_simd_ctx_create", C.c_int, [vp, C.c_uint64, C.POINTER(vp)]),
    ("fhe_simd_ctx_destroy", None, [vp]),
    ("fhe_simd_ctx_get_info", C.c_int, [vp, C.POINTER(SimdInfo)]),
    ("fhe_simd_slot_index", C.c_int, [vp, C.POINTER(C.c_uint32)]),
    ("fhe_simd_rotation_element", C.c_int, [C.c_uint32, C.c_int64, C.c_int, C.POINTER(C.c_uint32)]),
    ("fhe_simd_encode_batch", C.c_int, [vp, vp, C.c_int, vp, C.c_size_t, C.c_int]),
    ("fhe_simd_decode_batch", C.c_int, [vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_ct_galois_chain_batch", C.c_int,
     [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), vp, vp, C.c_int, vp,
      C.c_size_t, C.c_int]),
    ("fhe_ct_hoist_batch", C.c_int, [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_ct_hoisted_galois_batch", C.c_int,
     [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_ct_hoisted_linear_batch", C.c_int,
     [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), vp, vp, vp, C.c_int, vp, C.c_size_t,
      C.c_int]),
    ("fhe_glwe_rotate_batch", C.c_int, [vp, C.c_uint32, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_cmux_batch", C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_blind_rotate_batch", C.c_int,
     [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_sample_extract_batch", C.c_int, [vp, C.c_uint32, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_br_repair_count", C.c_int, [vp, C.POINTER(C.c_uint64)]),
    ("fhe_key_switch_batch", C.c_int,
     [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, C.c_size_t, C.c_int,
      C.c_int, vp]),
    ("fhe_slot_extract_batch", C.c_int,
     [vp, vp, vp, C.c_size_t, C.c_int, C.POINTER(C.c_uint32), u64p, C.c_size_t, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_lwe_sum_batch", C.c_int,
     [C.c_uint64, C.c_uint32, vp, vp, C.c_size_t, C.c_uint64, vp, vp, C.c_size_t, C.c_int, C.c_int, vp]),
    ("fhe_secret_key_prepare", C.c_int, [vp, vp, vp, C.c_int]),
    ("fhe_public_key_prepare", C.c_int, [vp, vp, vp, C.c_int]),
    ("fhe_encrypt_batch", C.c_int, [vp, C.c_uint64, vp, vp, vp, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_decrypt_batch", C.c_int,
     [vp, C.c_uint64, vp, vp, C.c_uint32, C.c_int, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_add_plain_batch", C.c_int, [vp, C.c_uint64, vp, vp, C.c_int, vp, C.c_size_t, C.c_int]),
    ("fhe_shamir_shares_batch", C.c_int, [vp, vp, C.c_uint32, C.c_uint32, vp, C.c_int]),
    ("fhe_key_share_prepare", C.c_int, [vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_partial_decrypt_batch", C.c_int, [vp, vp, C.c_size_t, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_lagrange_coefficients", C.c_int, [C.c_uint64, C.POINTER(C.c_uint32), C.c_size_t, C.c_size_t, u64p]),
    ("fhe_combine_partials_batch", C.c_int,
     [vp, C.c_uint64, vp, vp, u64p, C.c_size_t, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_bootstrap_batch", C.c_int,
     [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64, vp, vp, C.c_uint32, C.c_uint32,
      C.c_uint32, vp, vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_sample_batch", C.c_int, [vp, C.c_int, u64p, C.c_uint64, C.c_double, vp, C.c_size_t, C.c_int]),
    ("fhe_encrypt_sampled_batch", C.c_int,
     [vp, C.c_uint64, vp, vp, u64p, C.c_uint64, C.c_double, vp, C.c_size_t, C.c_int]),
    ("fhe_public_key_generate", C.c_int, [vp, vp, u64p, C.c_uint64, C.c_double, vp, C.c_int]),
    ("fhe_eval_key_generate", C.c_int, [vp, vp, C.c_uint32, C.c_uint32, u64p, C.c_uint64, C.c_double, vp, C.c_int]),
    ("fhe_ggsw_encrypt_batch", C.c_int,
     [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, u64p, C.c_uint64, C.c_double, vp, C.c_int]),
    ("fhe_ksk_generate", C.c_int,
     [vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, u64p, C.c_uint64, C.c_double, vp, vp, C.c_int]),
    ("fhe_pack_key_generate", C.c_int,
     [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, u64p, C.c_uint64, C.c_double, vp, C.c_int]),
    ("fhe_lwe_pack_batch", C.c_int,
     [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.POINTER(C.c_uint32), C.c_size_t, C.c_int, vp, C.c_size_t,
      C.c_int]),
    ("fhe_lwe_decrypt_batch", C.c_int,
     [C.c_uint64, C.c_uint64, vp, C.c_uint32, vp, vp, vp, vp, C.c_size_t, C.c_int, C.c_int, vp]),
    ("fhe_modmul_batch", C.c_int, [C.c_uint64, vp, vp, vp, C.c_size_t, C.c_int, C.c_int, vp]),
    ("fhe_ml_constants", C.c_int, [u64p, u64p]),
    ("fhe_ml_montmul_batch", C.c_int, [u64p, vp, vp, vp, C.c_size_t, C.c_int, C.c_int, vp]),
    ("fhe_mont_constants_compat", C.c_int, [C.c_uint64, u64p]),
    ("fhe_compat_montgomery_mul", C.c_uint64, [u64p, C.c_uint64, C.c_uint64]),
    ("fhe_compat_to_montgomery", C.c_uint64, [u64p, C.c_uint64]),
    ("fhe_compat_from_montgomery", C.c_uint64, [u64p, C.c_uint64]),
    ("fhe_compat_mod_add", C.c_uint64, [C.c_uint64, C.c_uint64, C.c_uint64]),
    ("fhe_compat_mod_sub", C.c_uint64, [C.c_uint64, C.c_uint64, C.c_uint64]),
    ("fhe_ctx_alloc", C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
    ("fhe_ctx_free", C.c_int, [vp, vp]),
    ("fhe_ctx_memcpy", C.c_int, [vp, vp, vp, C.c_size_t, C.c_int]),
    ("fhe_dev_alloc", C.c_int, [C.c_int, C.c_size_t, C.POINTER(vp)]),
    ("fhe_dev_free", C.c_int, [vp]),
    ("fhe_memcpy_h2d", C.c_int, [vp, vp, C.c_size_t]),
    ("fhe_memcpy_d2h", C.c_int, [vp, vp, C.c_size_t]),
    ("fhe_device_synchronize", C.c_int, [C.c_int]),
    ("fhe_event_create", C.c_int, [C.POINTER(vp)]),
    ("fhe_event_destroy", C.c_int, [vp]),
    ("fhe_event_record", C.c_int, [vp, vp]),
    ("fhe_event_elapsed_ms", C.c_int, [vp, vp, C.POINTER(C.c_float)]),
]

_lib = None


def lib():
    """Load libfhe_gpu.so (raises if it was not built: there is no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FHEError(-11, f"libfhe_gpu.so not found at {LIB_PATH}; run __graft_entry__.build()")
        L = C.CDLL(LIB_PATH)
        lab = "FHE_GPU_LIB" in os.environ  # lab A/B against an older build: skip its missing entries
        for name, res, args in SIGNATURES:
            if lab and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc: int):
    if rc != FHE_OK:
        raise FHEError(rc, lib().fhe_last_error().decode(errors="replace"))


def version() -> str:
    return lib().fhe_version().decode()


def build_id() -> str:
    """Hash of the sources and flags of the loaded library (Makefile)."""
    return lib().fhe_build_id().decode()


def detect_hardware() -> dict:
    """HardwareDetector::detect() / N-API detectHardware() for the MI355X."""
    caps = HwCaps()
    _check(lib().fhe_detect(C.byref(caps)))
    return {
        "deviceCount": caps.device_count, "computeUnits": caps.compute_units,
        "wavefrontSize": caps.wavefront_size, "xcds": caps.xcds, "hbmBytes": caps.hbm_bytes,
        "ldsBytesPerCu": caps.lds_bytes_per_cu, "arch": caps.arch.decode(), "name": caps.name.decode(),
    }


# ----------------------------------------------------------------- buffers
def _is_tensor(x) -> bool:
    return _HAVE_TORCH and isinstance(x, torch.Tensor)


def _stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class _Buf:
    """Pointer + placement for one argument."""

    __slots__ = ("ptr", "where", "count", "keep", "device")

    def __init__(self, x, writable=False):
        if _is_tensor(x):
            if not x.is_cuda:
                raise FHEError(-9, "torch tensors must be on a GPU (use numpy arrays for host data)")
            if x.dtype not in (torch.int64, torch.uint64):
                raise FHEError(-9, "device buffers must be int64/uint64 tensors")
            if not x.is_contiguous():
                raise FHEError(-9, "device buffers must be contiguous")
            self.ptr, self.where, self.count, self.keep = x.data_ptr(), FHE_DEVICE, x.numel(), x
            self.device = x.device
        else:
            a = x
            if not (isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]):
                if writable:
                    raise FHEError(-9, "output must be a C-contiguous numpy uint64 array")
                a = np.ascontiguousarray(np.asarray(x, dtype=np.uint64))
            self.ptr, self.where, self.count, self.keep = a.ctypes.data, FHE_HOST, a.size, a
            self.device = None


_TLS = threading.local()  # device of the last _where() call's tensors (for _bind_stream)


def _where(*bufs: _Buf) -> int:
    w = {b.where for b in bufs if b is not None}
    if len(w) != 1:
        raise FHEError(-9, "all buffers of one call must be host arrays or all device tensors")
    devs = {b.device for b in bufs if b is not None and b.device is not None}
    if len(devs) > 1:
        raise FHEError(-9, "all device tensors of one call must be on the same GPU")
    _TLS.device = devs.pop() if devs else None
    return w.pop()


def _like(x):
    if _is_tensor(x):
        return torch.empty_like(x)
    return np.empty(np.shape(x), dtype=np.uint64)


def _as_u64(x):
    if _is_tensor(x):
        return x
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64))


# ----------------------------------------------------------------- static helpers
def is_power_of_two(n: int) -> bool:  # ntt_processor.cpp:25-27
    return n > 0 and (n & (n - 1)) == 0


def log2_pow2(n: int) -> int:  # :29-36
    r = 0
    while n > 1:
        n >>= 1
        r += 1
    return r


def bit_reverse(index: int, bits: int) -> int:  # :38-45
    r = 0
    for _ in range(bits):
        r = (r << 1) | (index & 1)
        index >>= 1
    return r


def mod_pow(base: int, exp: int, mod: int) -> int:  # :47-62
    return pow(base % mod, exp, mod) if mod != 1 else 0


def mod_inverse(a: int, m: int) -> int:  # :64-90 (signed extended Euclid)
    if m == 0:
        raise FHEError(-8, "Modulus cannot be zero")
    if m == 1:
        return 0
    return pow(a % m, -1, m)


def find_primitive_root(degree: int, modulus: int) -> int:  # :92-128
    two_n = 2 * degree
    if (modulus - 1) % two_n:
        raise FHEError(-4, "Modulus is not NTT-friendly: q ≢ 1 (mod 2N)")
    e = (modulus - 1) // two_n
    for g in range(2, min(modulus, 1 << 22)):
        w = pow(g, e, modulus)
        if pow(w, two_n, modulus) == 1 and pow(w, degree, modulus) == modulus - 1:
            return w
    raise FHEError(-6, "Could not find primitive root for given parameters")


# ----------------------------------------------------------------- NTT / ring
def env_defaults(mode=None, device=None, devices=None):
    """Context defaults from the environment (SURVEY.md section 5 config flags):
    FHE_NTT_MODE = compat | negacyclic (mode when not given);
    FHE_GPU_DEVICES = comma-separated GPU ordinals (device list when neither
    device nor devices is given: one entry -> that device, several -> a
    multi-device context).  Returns (mode, device, devices)."""
    if mode is None:
        mode = os.environ.get("FHE_NTT_MODE", "compat").strip() or "compat"
    if device is None and devices is None:
        env = os.environ.get("FHE_GPU_DEVICES", "").strip()
        if env:
            try:
                devs = [int(x) for x in env.split(",") if x.strip()]
            except ValueError:
                raise FHEError(-9, f"FHE_GPU_DEVICES must be a comma-separated list of ordinals, got {env!r}")
            if len(devs) == 1:
                device = devs[0]
            elif devs:
                devices = devs
    if device is None:
        device = int(devices[0]) if devices else 0
    return mode, device, devices


class NTTProcessor:
    """NTTProcessor(degree, modulus) on the MI355X (ntt_processor.h:49-306).

    ``mode='compat'`` reproduces the reference transform bit for bit;
    ``mode='negacyclic'`` is the psi-twisted transform whose pointwise product
    is multiplication mod X^N + 1.
    """

    is_power_of_two = staticmethod(is_power_of_two)
    log2_pow2 = staticmethod(log2_pow2)
    bit_reverse = staticmethod(bit_reverse)
    mod_pow = staticmethod(mod_pow)
    mod_inverse = staticmethod(mod_inverse)
    find_primitive_root = staticmethod(find_primitive_root)

    def __init__(self, degree: int, modulus: int, mode: str = None, device: int = None, devices=None):
        """devices: a list of GPU ordinals for a multi-device context
        (fhe_ctx_create_multi): host-array batches are split across them, a
        device tensor runs on the GPU that holds it.  Unset arguments come
        from the environment (env_defaults): mode from FHE_NTT_MODE, the
        device list from FHE_GPU_DEVICES; otherwise compat on device 0."""
        mode, device, devices = env_defaults(mode, device, devices)
        m = {"compat": MODE_COMPAT, "negacyclic": MODE_NEGACYCLIC}.get(mode)
        if m is None:
            raise FHEError(-9, f"unknown mode {mode!r}")
        h = C.c_void_p()
        if devices is not None:
            devs = [int(d) for d in devices]
            arr = (C.c_int * max(1, len(devs)))(*devs)
            _check(lib().fhe_ctx_create_multi(degree, modulus, m, arr, len(devs), C.byref(h)))
            device = devs[0]
        else:
            _check(lib().fhe_ctx_create(degree, modulus, m, device, C.byref(h)))
        self._h = h
        self.devices = list(devices) if devices is not None else [device]
        self.degree, self.modulus, self.mode, self.device = degree, modulus, mode, device
        info = CtxInfo()
        _check(lib().fhe_ctx_get_info(h, C.byref(info)))
        self.info = info

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and _lib is not None:
            _lib.fhe_ctx_destroy(h)
        self._h = None

    __del__ = close

    # -- introspection (get_degree/get_modulus/get_twiddles, ntt_processor.h)
    def get_degree(self):
        return self.degree

    def get_modulus(self):
        return self.modulus

    @property
    def primitive_root(self):
        return self.info.psi

    @property
    def inv_n(self):
        return self.info.inv_n

    def get_twiddles(self):
        f = np.empty(self.degree, dtype=np.uint64)
        i = np.empty(self.degree, dtype=np.uint64)
        _check(lib().fhe_ctx_get_twiddles(self._h, f.ctypes.data, i.ctypes.data))
        return {"forward": f, "inverse": i, "primitive_root": self.info.psi, "inv_n": self.info.inv_n}

    # -- plumbing
    def _batch(self, x) -> int:
        shape = tuple(x.shape)
        if not shape or shape[-1] != self.degree:
            raise FHEError(-5, "Coefficient count must equal polynomial degree")
        b = 1
        for s in shape[:-1]:
            b *= s
        return b

    def _bind_stream(self, where):
        if where == FHE_DEVICE:
            _check(lib().fhe_ctx_set_stream(self._h, _stream_ptr(getattr(_TLS, "device", None))))

    def _unary(self, fn, x, out):
        x = _as_u64(x)
        nb = self._batch(x)
        out = _like(x) if out is None else out
        bi, bo = _Buf(x), _Buf(out, True)
        w = _where(bi, bo)
        self._bind_stream(w)
        _check(fn(self._h, bi.ptr, bo.ptr, nb, w))
        return out

    def _binary(self, fn, a, b, out):
        a, b = _as_u64(a), _as_u64(b)
        nb = self._batch(a)
        if tuple(b.shape) != tuple(a.shape):
            raise FHEError(-9, "operand shapes differ")
        out = _like(a) if out is None else out
        ba, bb, bo = _Buf(a), _Buf(b), _Buf(out, True)
        w = _where(ba, bb, bo)
        self._bind_stream(w)
        _check(fn(self._h, ba.ptr, bb.ptr, bo.ptr, nb, w))
        return out

    # -- transforms
    def forward_ntt(self, coeffs, out=None):
        """forward_ntt (ntt_processor.cpp:262-319); pass out=coeffs for in place."""
        return self._unary(lib().fhe_ntt_fwd_batch, coeffs, out)

    def inverse_ntt(self, coeffs, out=None):
        """inverse_ntt (ntt_processor.cpp:325-388)."""
        return self._unary(lib().fhe_ntt_inv_batch, coeffs, out)

    forward_ntt_batch = forward_ntt
    inverse_ntt_batch = inverse_ntt

    def forward_ntt_mul(self, coeffs, w, out=None):
        """to_ntt(coeffs) then pointwise by w (config C3, fused)."""
        return self._binary(lib().fhe_ntt_fwd_mul_batch, coeffs, w, out)

    # -- public integer weights
    def sum_scaled(self, cts, scalars, out=None, accumulate: bool = False, grouped=None):
        """sum_i cts[i] * scalars[i] over the ballot axis in one launch
        (multiply_scalar per ballot folded by add()): cts [count, ..., n] with
        scalars [count], or cts [groups, count, ..., n] with scalars
        [groups, count]; `...` is empty or the 1..3 polynomials of a
        ciphertext.  Shapes as sum_batch; words and scalars are any u64.
        accumulate: `out` is one more (unscaled) term of each sum."""
        cts = _as_u64(cts)
        shape = tuple(cts.shape)
        grouped = len(shape) == 4 if grouped is None else bool(grouped)
        lead = 2 if grouped else 1
        if len(shape) < lead + 1 or shape[-1] != self.degree:
            raise FHEError(-5, "Coefficient count must equal polynomial degree")
        groups, count = (shape[0], shape[1]) if grouped else (1, shape[0])
        if not _is_tensor(scalars):
            scalars = np.ascontiguousarray(np.asarray(scalars, dtype=np.uint64))
            if _is_tensor(cts):
                scalars = torch.from_numpy(scalars.view(np.int64)).to(cts.device)
        if tuple(scalars.shape) != shape[:lead]:
            raise FHEError(-9, "Ballots and weights must have the same size")
        polys = 1
        for d in shape[lead:-1]:
            polys *= d
        oshape = ((groups,) if grouped else ()) + shape[lead:]
        if out is None:
            if accumulate:
                raise FHEError(-9, "accumulate needs an out buffer")
            out = _empty(cts, oshape)
        elif tuple(out.shape) != oshape:
            raise FHEError(-9, f"out must have shape {list(oshape)}")
        ba, bs, bo = _Buf(cts), _Buf(scalars), _Buf(out, True)
        w = _where(ba, bs, bo)
        self._bind_stream(w)
        _check(lib().fhe_ct_sum_scaled_batch(self._h, ba.ptr, bs.ptr, polys, count, groups, int(bool(accumulate)),
                                             bo.ptr, w))
        return out

    def sum_scaled_buffers(self, bufs, scalars, out=None, accumulate: bool = False):
        """sum_scaled over separately allocated device tensors [..., n] of one
        shape (1..3 polynomials each) and a host sequence of integer scalars;
        a tensor may be listed twice."""
        bufs = list(bufs)
        scal = np.ascontiguousarray(np.asarray([int(s) & (2**64 - 1) for s in scalars], dtype=np.uint64))
        if len(scal) != len(bufs):
            raise FHEError(-9, "Ballots and weights must have the same size")
        if not bufs:
            raise FHEError(-9, "Cannot add empty vector of ciphertexts")
        shape = tuple(bufs[0].shape)
        if not shape or shape[-1] != self.degree:
            raise FHEError(-5, "Coefficient count must equal polynomial degree")
        if any(tuple(b.shape) != shape for b in bufs):
            raise FHEError(-9, "operand shapes differ")
        polys = 1
        for d in shape[:-1]:
            polys *= d
        if out is None:
            if accumulate:
                raise FHEError(-9, "accumulate needs an out buffer")
            out = torch.empty_like(bufs[0])
        bs, bo = [_Buf(b) for b in bufs], _Buf(out, True)
        if _where(bo, *bs) != FHE_DEVICE:
            raise FHEError(-9, "sum_scaled_buffers takes device tensors (stack host arrays for sum_scaled)")
        self._bind_stream(FHE_DEVICE)
        table = (C.c_void_p * len(bs))(*[b.ptr for b in bs])
        _check(lib().fhe_ct_sum_scaled_ptrs(self._h, table, scal.ctypes.data, polys, len(bs), int(bool(accumulate)),
                                            bo.ptr))
        return out


class PolynomialRing(NTTProcessor):
    """PolynomialRing(degree, modulus) (polynomial_ring.h:101-516) over batches."""

    def multiply(self, a, b, out=None):
        """multiply (polynomial_ring.cpp:421-447): inv(fwd(a) (.) fwd(b)), fused."""
        return self._binary(lib().fhe_polymul_batch, a, b, out)

    def pointwise_multiply(self, a, b, out=None):
        return self._binary(lib().fhe_pointwise_batch, a, b, out)

    def add(self, a, b, out=None):
        return self._binary(lib().fhe_poly_add_batch, a, b, out)

    def subtract(self, a, b, out=None):
        return self._binary(lib().fhe_poly_sub_batch, a, b, out)

    def negate(self, a, out=None):
        return self._unary(lib().fhe_poly_neg_batch, a, out)

    def galois(self, p, g: int, out=None):
        """sigma_g, the automorphism X -> X^g (g odd, below 2n) of [..., n]
        polynomials (fhe_poly_galois_batch): a signed permutation, canonical
        output, out of place."""
        p = _as_u64(p)
        nb = self._batch(p)
        out = _like(p) if out is None else out
        bi, bo = _Buf(p), _Buf(out, True)
        w = _where(bi, bo)
        self._bind_stream(w)
        _check(lib().fhe_poly_galois_batch(self._h, int(g), bi.ptr, bo.ptr, nb, w))
        return out

    def multiply_scalar(self, a, scalar: int, out=None):
        a = _as_u64(a)
        nb = self._batch(a)
        out = _like(a) if out is None else out
        ba, bo = _Buf(a), _Buf(out, True)
        w = _where(ba, bo)
        self._bind_stream(w)
        _check(lib().fhe_poly_mul_scalar_batch(self._h, ba.ptr, scalar, bo.ptr, nb, w))
        return out

    def sum_batch(self, a, out=None, accumulate: bool = False, grouped=None):
        """Sum over the ballot axis in one launch (batch_add / batch_add_tree,
        encryption.cpp:1327-1460): a [count, ..., n] -> [..., n], or
        a [groups, count, ..., n] -> [groups, ..., n]; `...` is empty or the
        1..3 polynomials of a ciphertext.  grouped=None reads a 4-d input as
        grouped.  accumulate: `out` is one more term of each sum."""
        a = _as_u64(a)
        shape = tuple(a.shape)
        grouped = len(shape) == 4 if grouped is None else bool(grouped)
        lead = 2 if grouped else 1
        if len(shape) < lead + 1 or shape[-1] != self.degree:
            raise FHEError(-5, "Coefficient count must equal polynomial degree")
        groups, count = (shape[0], shape[1]) if grouped else (1, shape[0])
        polys = 1
        for d in shape[lead:-1]:
            polys *= d
        oshape = ((groups,) if grouped else ()) + shape[lead:]
        if out is None:
            if accumulate:
                raise FHEError(-9, "accumulate needs an out buffer")
            out = _empty(a, oshape)
        elif tuple(out.shape) != oshape:
            raise FHEError(-9, f"out must have shape {list(oshape)}")
        ba, bo = _Buf(a), _Buf(out, True)
        w = _where(ba, bo)
        self._bind_stream(w)
        _check(lib().fhe_ct_sum_batch(self._h, ba.ptr, polys, count, groups, int(bool(accumulate)), bo.ptr, w))
        return out

    def sum_buffers(self, bufs, out=None, accumulate: bool = False):
        """sum_batch over separately allocated device tensors [..., n] of one
        shape (1..3 polynomials each); a tensor may be listed twice."""
        bufs = list(bufs)
        if not bufs:
            raise FHEError(-9, "Cannot add empty vector of ciphertexts")
        shape = tuple(bufs[0].shape)
        if not shape or shape[-1] != self.degree:
            raise FHEError(-5, "Coefficient count must equal polynomial degree")
        if any(tuple(b.shape) != shape for b in bufs):
            raise FHEError(-9, "operand shapes differ")
        polys = 1
        for d in shape[:-1]:
            polys *= d
        if out is None:
            if accumulate:
                raise FHEError(-9, "accumulate needs an out buffer")
            out = torch.empty_like(bufs[0])
        bs, bo = [_Buf(b) for b in bufs], _Buf(out, True)
        if _where(bo, *bs) != FHE_DEVICE:
            raise FHEError(-9, "sum_buffers takes device tensors (stack host arrays for sum_batch)")
        self._bind_stream(FHE_DEVICE)
        table = (C.c_void_p * len(bs))(*[b.ptr for b in bs])
        _check(lib().fhe_ct_sum_ptrs(self._h, table, polys, len(bs), int(bool(accumulate)), bo.ptr))
        return out

    def to_ntt(self, p, out=None):
        return self.forward_ntt(p, out)

    def from_ntt(self, p, out=None):
        return self.inverse_ntt(p, out)


class RNSPolynomialRing:
    """PolynomialRing(degree, moduli) (polynomial_ring.cpp:224-237): one
    transform context per modulus on one stream.  Arrays are modulus-major
    [len(moduli), ..., n]; every operation applies to every limb (the
    reference's ring operations use moduli_[0] only)."""

    def __init__(self, degree: int, moduli, mode: str = None, device: int = None):
        mode, device, devs = env_defaults(mode, device, None)  # one device: the first of FHE_GPU_DEVICES
        m = {"compat": MODE_COMPAT, "negacyclic": MODE_NEGACYCLIC}.get(mode)
        if m is None:
            raise FHEError(-9, f"unknown mode {mode!r}")
        mods = [int(x) for x in moduli]
        arr = (C.c_uint64 * max(1, len(mods)))(*mods)
        h = C.c_void_p()
        _check(lib().fhe_rns_ctx_create(degree, arr, len(mods), m, device, C.byref(h)))
        self._h = h
        self.degree, self.moduli, self.mode, self.device = degree, mods, mode, device

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and _lib is not None:
            _lib.fhe_rns_ctx_destroy(h)
        self._h = None

    __del__ = close

    def _batch(self, x) -> int:
        shape = tuple(x.shape)
        if len(shape) < 2 or shape[0] != len(self.moduli) or shape[-1] != self.degree:
            raise FHEError(-5, f"RNS arrays must be [{len(self.moduli)}, ..., {self.degree}]")
        return int(np.prod(shape[1:-1])) if len(shape) > 2 else 1

    def _bind(self, where):
        if where == FHE_DEVICE:
            first = C.c_void_p()
            _check(lib().fhe_rns_ctx_limb(self._h, 0, C.byref(first)))
            _check(lib().fhe_ctx_set_stream(first, _stream_ptr()))
            for i in range(1, len(self.moduli)):
                c = C.c_void_p()
                _check(lib().fhe_rns_ctx_limb(self._h, i, C.byref(c)))
                _check(lib().fhe_ctx_set_stream(c, _stream_ptr()))

    def _unary(self, fn, x, out):
        x = _as_u64(x)
        nb = self._batch(x)
        out = _like(x) if out is None else out
        bi, bo = _Buf(x), _Buf(out, True)
        w = _where(bi, bo)
        self._bind(w)
        _check(fn(self._h, bi.ptr, bo.ptr, nb, w))
        return out

    def _binary(self, fn, a, b, out):
        a, b = _as_u64(a), _as_u64(b)
        nb = self._batch(a)
        if tuple(b.shape) != tuple(a.shape):
            raise FHEError(-9, "operand shapes differ")
        out = _like(a) if out is None else out
        ba, bb, bo = _Buf(a), _Buf(b), _Buf(out, True)
        w = _where(ba, bb, bo)
        self._bind(w)
        _check(fn(self._h, ba.ptr, bb.ptr, bo.ptr, nb, w))
        return out

    def forward_ntt(self, x, out=None):
        return self._unary(lib().fhe_rns_ntt_fwd_batch, x, out)

    def inverse_ntt(self, x, out=None):
        return self._unary(lib().fhe_rns_ntt_inv_batch, x, out)

    def multiply(self, a, b, out=None):
        return self._binary(lib().fhe_rns_polymul_batch, a, b, out)

    def pointwise_multiply(self, a, b, out=None):
        return self._binary(lib().fhe_rns_pointwise_batch, a, b, out)

    def add(self, a, b, out=None):
        return self._binary(lib().fhe_rns_add_batch, a, b, out)

    def subtract(self, a, b, out=None):
        return self._binary(lib().fhe_rns_sub_batch, a, b, out)


class ExternalProduct:
    """BootstrapEngine::external_product (bootstrap_engine.cpp:431-518) for a
    batch of GLWE ciphertexts ([..., k+1, n]) against one GGSW
    ([(k+1)*level, k+1, n], coefficient form, reference row order)."""

    def __init__(self, ring: NTTProcessor, ggsw, base_log: int, level: int, k: int = 1):
        self.ring, self.base_log, self.level, self.k = ring, base_log, level, k
        g = _as_u64(ggsw)
        exp = ((k + 1) * level, k + 1, ring.degree)
        if tuple(g.shape) != exp:
            raise FHEError(-9, f"ggsw shape must be {exp}")
        self.ggsw_ntt = _like(g)
        bi, bo = _Buf(g), _Buf(self.ggsw_ntt, True)
        w = _where(bi, bo)
        ring._bind_stream(w)
        _check(lib().fhe_ggsw_prepare(ring._h, k, level, bi.ptr, bo.ptr, w))

    def __call__(self, glwe, out=None):
        glwe = _as_u64(glwe)
        shape = tuple(glwe.shape)
        if len(shape) < 2 or shape[-2:] != (self.k + 1, self.ring.degree):
            raise FHEError(-9, "glwe must have shape [..., k+1, n]")
        nb = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
        out = _like(glwe) if out is None else out
        bi, bk, bo = _Buf(glwe), _Buf(self.ggsw_ntt), _Buf(out, True)
        w = _where(bi, bk, bo)
        self.ring._bind_stream(w)
        _check(lib().fhe_external_product_batch(self.ring._h, self.k, self.base_log, self.level, bi.ptr, bk.ptr,
                                                bo.ptr, nb, w))
        return out


def _empty(like, shape):
    if _is_tensor(like):
        return torch.empty(shape, dtype=like.dtype, device=like.device)
    return np.empty(shape, dtype=np.uint64)


def _lead(x, tail) -> int:
    """Batch size of x with trailing shape `tail`."""
    shape = tuple(x.shape)
    if len(shape) < len(tail) or shape[len(shape) - len(tail):] != tuple(tail):
        raise FHEError(-9, f"expected shape [..., {', '.join(map(str, tail))}], got {list(shape)}")
    return int(np.prod(shape[: len(shape) - len(tail)])) if len(shape) > len(tail) else 1


class EvaluationKey:
    """Relinearisation key (KeySwitchKey of key_manager.h:85-111): the
    (a_l, b_l) pairs ``rlk`` [level, 2, n] in coefficient form, prepared once
    into the NTT domain on the GPU."""

    def __init__(self, ring: "PolynomialRing", rlk, decomp_base_log: int = 0):
        rlk = _as_u64(rlk)
        self.level = int(rlk.shape[0]) if rlk.ndim == 3 else 0
        if self.level and tuple(rlk.shape[1:]) != (2, ring.degree):
            raise FHEError(-9, "rlk must have shape [level, 2, n]")
        # encryption.cpp:935: base_log 0 -> 4
        self.decomp_base_log = decomp_base_log if decomp_base_log > 0 else 4
        self.ring = ring
        self.rlk_ntt = _like(rlk)
        if self.level:
            bi, bo = _Buf(rlk), _Buf(self.rlk_ntt, True)
            w = _where(bi, bo)
            ring._bind_stream(w)
            _check(lib().fhe_relin_key_prepare(ring._h, self.level, bi.ptr, bo.ptr, w))


class SwitchKey:
    """Key-switching key(s) of fhe_ct_galois_batch / fhe_ct_trace_batch
    (KeyGenerator.switch_key, KeyGenerator.galois_keys): the raw (a_l, b_l)
    pairs ``key`` [level, 2, n] (or [steps, level, 2, n], key i for
    ``g[i]``), the decomposition, the Galois element(s) ``g`` and the
    NTT-domain form ``key_ntt``, prepared on first use."""

    def __init__(self, ring: "PolynomialRing", key, base_log: int, level: int, g=1):
        key = _as_u64(key)
        if tuple(key.shape[-3:]) != (level, 2, ring.degree) or len(key.shape) not in (3, 4):
            raise FHEError(-9, "switch key must have shape [level, 2, n] or [steps, level, 2, n]")
        self.ring, self.key, self.base_log, self.level, self.g = ring, key, int(base_log), int(level), g
        self.steps = int(key.shape[0]) if len(key.shape) == 4 else None
        self._ntt = None

    @property
    def key_ntt(self):
        if self._ntt is None:
            out = _like(self.key)
            if self.level:
                bi, bo = _Buf(self.key), _Buf(out, True)
                w = _where(bi, bo)
                self.ring._bind_stream(w)
                _check(lib().fhe_relin_key_prepare(self.ring._h, self.level * (self.steps or 1), bi.ptr, bo.ptr, w))
            self._ntt = out
        return self._ntt


class HoistedCiphertext:
    """A ciphertext decomposed and transformed once (EncryptionEngine.hoist,
    fhe_ct_hoist_batch): ``buf`` [..., 1 + level, n] holds the spectrum of c0
    and of the `level` unsigned base-2^base_log digits of c1.  ``ct`` is the
    ciphertext it came from (the unrotated term of a linear transform needs
    it)."""

    def __init__(self, ring: "PolynomialRing", buf, base_log: int, level: int, ct=None):
        buf = _as_u64(buf)
        if len(buf.shape) < 2 or tuple(buf.shape[-2:]) != (1 + int(level), ring.degree):
            raise FHEError(-9, "hoisted buffer must have shape [..., 1 + level, n]")
        self.ring, self.buf, self.base_log, self.level, self.ct = ring, buf, int(base_log), int(level), ct


class PreparedPlaintext:
    """One plaintext of a linear transform, already encoded and lifted
    (EncryptionEngine.prepare_plain): ``coeff`` [n] the polynomial (what the
    unrotated term multiplies by), ``row`` [n] its transform (what the rotated
    terms multiply by).  Host arrays or device tensors; they stay where they
    are."""

    def __init__(self, row, coeff):
        self.row, self.coeff = _as_u64(row), _as_u64(coeff)


class SecretKey:
    """SecretKey (key_manager.h): the polynomial s [n] and its NTT-domain
    form prepared once on the GPU (fhe_secret_key_prepare: s and s^2)."""

    def __init__(self, ring: "PolynomialRing", poly):
        s = _as_u64(poly)
        if tuple(s.shape) != (ring.degree,):
            raise FHEError(-9, "secret key must have shape [n]")
        self.poly, self.ring = s, ring
        self.prep = _empty(s, (2, ring.degree))
        bi, bo = _Buf(s), _Buf(self.prep, True)
        w = _where(bi, bo)
        ring._bind_stream(w)
        _check(lib().fhe_secret_key_prepare(ring._h, bi.ptr, bo.ptr, w))


class PublicKey:
    """PublicKey (key_manager.h:70-76): (a, b = a s + e) as [2, n], prepared
    once into the NTT domain (fhe_public_key_prepare)."""

    def __init__(self, ring: "PolynomialRing", a, b=None):
        pk = _as_u64(a) if b is None else (torch.stack([_as_u64(a), _as_u64(b)]) if _is_tensor(a)
                                            else np.stack([_as_u64(a), _as_u64(b)]))
        if tuple(pk.shape) != (2, ring.degree):
            raise FHEError(-9, "public key must have shape [2, n] = (a, b)")
        self.poly, self.ring = pk, ring
        self.prep = _like(pk)
        bi, bo = _Buf(pk), _Buf(self.prep, True)
        w = _where(bi, bo)
        ring._bind_stream(w)
        _check(lib().fhe_public_key_prepare(ring._h, bi.ptr, bo.ptr, w))


def _placed_like(x, like):
    """x on the side of `like` (host array or device tensor)."""
    if _is_tensor(like) and not _is_tensor(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).to(like.device)
    if _is_tensor(x) and not _is_tensor(like):
        return x.cpu().numpy().view(np.uint64)
    return x


def lagrange_coefficients(q: int, share_ids, used=None):
    """KeyManager::lagrange_coefficient (key_manager.cpp:548-582) at 0 for the
    first ``used`` of ``share_ids`` (default: all), interpolating over every
    id given (fhe_lagrange_coefficients; needs no GPU)."""
    ids = [int(i) for i in share_ids]
    used = len(ids) if used is None else int(used)
    if any(not 0 <= i < 1 << 32 for i in ids):
        raise FHEError(-9, "share ids must be 32-bit unsigned integers")
    arr = (C.c_uint32 * max(len(ids), 1))(*ids)
    out = (C.c_uint64 * max(used, 1))()
    _check(lib().fhe_lagrange_coefficients(int(q), arr, len(ids), max(used, 0), out))
    return [int(out[i]) for i in range(used)]


def shamir_shares(ring: "NTTProcessor", coeffs, total_shares: int, out=None):
    """The Shamir evaluation of generate_threshold_keys (key_manager.cpp:
    511-526): coeffs [threshold, n] -> shares [total_shares, n] at the points
    1..total_shares (fhe_shamir_shares_batch)."""
    coeffs = _as_u64(coeffs)
    if len(coeffs.shape) != 2 or coeffs.shape[1] != ring.degree:
        raise FHEError(-9, "coeffs must have shape [threshold, n]")
    total_shares = int(total_shares)
    if out is None:
        out = _empty(coeffs, (max(total_shares, 0), ring.degree))
    bc, bo = _Buf(coeffs), _Buf(out, True)
    if bo.count != total_shares * ring.degree:
        raise FHEError(-9, "out must have shape [total_shares, n]")
    w = _where(bc, bo)
    ring._bind_stream(w)
    _check(lib().fhe_shamir_shares_batch(ring._h, bc.ptr, int(coeffs.shape[0]), total_shares, bo.ptr, w))
    return out


class KeyShare:
    """SecretKeyShare (key_manager.h): the share's id (its evaluation point)
    and polynomial [n]; the NTT-domain form partial decryption multiplies with
    is prepared on first use (fhe_key_share_prepare) and kept."""

    def __init__(self, ring: "PolynomialRing", share_id: int, poly):
        s = _as_u64(poly)
        if tuple(s.shape) != (ring.degree,):
            raise FHEError(-9, "a key share must have shape [n]")
        self.ring, self.share_id, self.poly = ring, int(share_id), s
        self._prep = None

    @property
    def prep(self):
        if self._prep is None:
            out = _like(self.poly)
            bi, bo = _Buf(self.poly), _Buf(out, True)
            w = _where(bi, bo)
            self.ring._bind_stream(w)
            _check(lib().fhe_key_share_prepare(self.ring._h, bi.ptr, bo.ptr, 1, w))
            self._prep = out
        return self._prep


class ThresholdKeys:
    """ThresholdKeys (key_manager.h): the trustees' shares, the master secret
    key they interpolate to (for dealers and tests), and the parameters."""

    def __init__(self, shares, secret_key, threshold: int, total_shares: int):
        self.shares, self.secret_key = list(shares), secret_key
        self.threshold, self.total_shares = int(threshold), int(total_shares)


SAMPLE_UNIFORM, SAMPLE_TERNARY, SAMPLE_GAUSSIAN, SAMPLE_BINARY, SAMPLE_RAW = range(5)


def _seed_arr(seed):
    """A 256-bit ChaCha20 seed as 4 u64 words (an int, 4 ints, or bytes)."""
    if isinstance(seed, (bytes, bytearray)):
        seed = np.frombuffer(bytes(seed).ljust(32, b"\0")[:32], dtype=np.uint64)
    elif isinstance(seed, int):
        seed = [(seed >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]
    a = (C.c_uint64 * 4)(*[int(x) for x in np.asarray(seed, dtype=np.uint64).reshape(4)])
    return a


def new_seed() -> bytes:
    """256 bits from the OS CSPRNG (the engine's default seed)."""
    return os.urandom(32)


def sample(ring: "NTTProcessor", kind: int, seed, stream: int, count: int, std_dev: float = 3.2, out=None,
           device_out: bool = False):
    """SecureRandom draws (key_manager.cpp:53-115) over the seeded ChaCha20
    stream of include/fhe_gpu.h (fhe_sample_batch), modulo the ring modulus."""
    if out is None:
        out = (torch.empty(count, dtype=torch.int64, device=f"cuda:{ring.device}") if device_out
               else np.empty(count, dtype=np.uint64))
    bo = _Buf(out, True)
    w = _where(bo)
    ring._bind_stream(w)
    _check(lib().fhe_sample_batch(ring._h, int(kind), _seed_arr(seed), int(stream), float(std_dev), bo.ptr, count, w))
    return out


class KeyGenerator:
    """KeyManager (key_manager.cpp:150-333) and the bootstrapping-key half of
    BootstrapEngine (bootstrap_engine.cpp:268-420) on the GPU, drawing from
    a seeded ChaCha20 stream: the same (seed, stream) gives the same keys on
    every device and in the CPU oracle.  Arrays follow the placement of the
    inputs (numpy: host, torch: device)."""

    def __init__(self, ring: "PolynomialRing", seed=None, noise_std: float = 3.2):
        self.ring = ring
        self.seed = seed if seed is not None else new_seed()
        self.noise_std = float(noise_std)

    def secret_key(self, stream: int, kind: int = SAMPLE_TERNARY, device_out: bool = False):
        """generate_secret_key (:150-196): TERNARY (default), GAUSSIAN, BINARY or UNIFORM coefficients."""
        return sample(self.ring, kind, self.seed, stream, self.ring.degree, self.noise_std, device_out=device_out)

    def public_key(self, sk, stream: int, out=None):
        """generate_public_key (:218-246) -> [2, n] = (a, a (*) s + e)."""
        r = self.ring
        sk = _as_u64(sk)
        out = _empty(sk, (2, r.degree)) if out is None else out
        bs, bo = _Buf(sk), _Buf(out, True)
        w = _where(bs, bo)
        r._bind_stream(w)
        _check(lib().fhe_public_key_generate(r._h, bs.ptr, _seed_arr(self.seed), stream, self.noise_std, bo.ptr, w))
        return out

    def eval_key(self, sk, base_log: int, level: int, stream: int, out=None):
        """generate_eval_key (:252-333) -> rlk [level, 2, n] (KeySwitchKey pairs (a_l, b_l))."""
        r = self.ring
        sk = _as_u64(sk)
        out = _empty(sk, (level, 2, r.degree)) if out is None else out
        bs, bo = _Buf(sk), _Buf(out, True)
        w = _where(bs, bo)
        r._bind_stream(w)
        _check(lib().fhe_eval_key_generate(r._h, bs.ptr, base_log, level, _seed_arr(self.seed), stream,
                                           self.noise_std, bo.ptr, w))
        return out

    def switch_key(self, sk_to, sk_from, base_log: int, level: int, stream: int, g: int = 1, out=None):
        """fhe_switch_key_generate -> SwitchKey over [level, 2, n]: switches
        sigma_g(ct) from sigma_g(sk_from) to sk_to.  g = 1 with two keys is a
        re-keying key, sk_from = sk_to with g != 1 a Galois key.  Streams
        stream .. stream + 2 level - 1."""
        r = self.ring
        st = _as_u64(sk_to.poly if isinstance(sk_to, SecretKey) else sk_to)
        sf = _as_u64(sk_from.poly if isinstance(sk_from, SecretKey) else sk_from)
        out = _empty(st, (level, 2, r.degree)) if out is None else out
        bt, bf, bo = _Buf(st), _Buf(sf), _Buf(out, True)
        if bo.count != level * 2 * r.degree:
            raise FHEError(-9, "switch key must be [level, 2, n]")
        w = _where(bt, bf, bo)
        r._bind_stream(w)
        _check(lib().fhe_switch_key_generate(r._h, bt.ptr, bf.ptr, int(g), base_log, level, _seed_arr(self.seed),
                                             stream, self.noise_std, bo.ptr, w))
        return SwitchKey(r, out, base_log, level, int(g))

    def galois_keys(self, sk, base_log: int, level: int, stream: int, steps=None):
        """The Galois keys of the trace in one buffer [steps, level, 2, n]:
        key i for g_i = n / 2^i + 1 on streams stream + 2 level i ...;
        steps defaults to log2(n), the full trace."""
        r = self.ring
        steps = r.degree.bit_length() - 1 if steps is None else int(steps)
        if steps < 1 or steps > r.degree.bit_length() - 1:
            raise FHEError(-9, "steps must be between 1 and log2(n)")
        s = _as_u64(sk.poly if isinstance(sk, SecretKey) else sk)
        out = _empty(s, (steps, level, 2, r.degree))
        gs = [(r.degree >> i) + 1 for i in range(steps)]
        for i, g in enumerate(gs):
            self.switch_key(s, s, base_log, level, stream + 2 * level * i, g, out=out[i])
        return SwitchKey(r, out, base_log, level, gs)

    def rotation_keys(self, sk, base_log: int, level: int, stream: int):
        """The Galois keys of the SIMD slot rotations in one buffer
        [log2 n, level, 2, n]: key i < log2(n/2) for g_i = 3^(2^i) mod 2n (rotate
        the rows left by 2^i), the last one for g = 2n - 1 (swap the rows) --
        the slot-sum list of include/fhe_gpu.h.  Key i on streams
        stream + 2 level i ..., as galois_keys."""
        return self._galois_key_set(sk, slot_sum_elements(self.ring.degree), base_log, level, stream)

    def _galois_key_set(self, sk, gs, base_log: int, level: int, stream: int):
        """One Galois key per element of gs in one buffer [len(gs), level, 2, n],
        key i on streams stream + 2 level i ...."""
        r = self.ring
        s = _as_u64(sk.poly if isinstance(sk, SecretKey) else sk)
        out = _empty(s, (len(gs), level, 2, r.degree))
        for i, g in enumerate(gs):
            self.switch_key(s, s, base_log, level, stream + 2 * level * i, g, out=out[i])
        return SwitchKey(r, out, base_log, level, gs)

    def rotation_keys_for(self, sk, steps, base_log: int, level: int, stream: int, swap_rows: bool = False):
        """One Galois key per requested row-rotation step in one buffer
        [len(steps), level, 2, n]: key i for g_i = rotation_element(n, steps[i],
        swap_rows), on streams stream + 2 level i ....  rotation_keys holds the
        power-of-two steps only; rotate_many / linear_transform / matvec look a
        step's key up by its element in the returned SwitchKey's g list."""
        gs = [rotation_element(self.ring.degree, int(st), swap_rows) for st in steps]
        if not gs:
            raise FHEError(-9, "at least one step is needed")
        return self._galois_key_set(sk, gs, base_log, level, stream)

    def threshold_keys(self, threshold: int, total_shares: int, stream: int, device_out: bool = False):
        """generate_threshold_keys (:479-546): a ternary master key from
        ``stream``, the random sharing polynomial j (1 <= j < threshold) from
        ``stream + j`` (uniform, n draws each), and the shares at the points
        1..total_shares (fhe_shamir_shares_batch) -> ThresholdKeys."""
        r = self.ring
        threshold, total_shares = int(threshold), int(total_shares)
        if threshold < 1 or threshold > total_shares:
            raise FHEError(-9, "Invalid threshold parameters")
        master = self.secret_key(stream, device_out=device_out)
        coeffs = _empty(master, (threshold, r.degree))
        coeffs[0] = master
        for j in range(1, threshold):
            sample(r, SAMPLE_UNIFORM, self.seed, stream + j, r.degree, out=coeffs[j])
        shares = shamir_shares(r, coeffs, total_shares)
        return ThresholdKeys([KeyShare(r, i + 1, shares[i]) for i in range(total_shares)], SecretKey(r, master),
                             threshold, total_shares)

    def ggsw(self, values, sk, k: int, base_log: int, level: int, stream: int, out=None):
        """encrypt_ggsw (bootstrap_engine.cpp:268-306) of int64 values ->
        [count, (k+1) level, k+1, n] coefficient form."""
        r = self.ring
        if _is_tensor(values):
            vals = values.to(torch.int64).contiguous()
        else:
            vals = np.ascontiguousarray(np.asarray(values, dtype=np.int64)).view(np.uint64)
        sk = _as_u64(sk)
        cnt = int(vals.numel() if _is_tensor(vals) else vals.size)
        out = _empty(sk, (cnt, (k + 1) * level, k + 1, r.degree)) if out is None else out
        bv, bs, bo = _Buf(vals), _Buf(sk), _Buf(out, True)
        w = _where(bv, bs, bo)
        r._bind_stream(w)
        _check(lib().fhe_ggsw_encrypt_batch(r._h, k, base_log, level, bv.ptr, cnt, bs.ptr, _seed_arr(self.seed),
                                            stream, self.noise_std, bo.ptr, w))
        return out

    def key_switch_key(self, glwe_sk, lwe_sk, base_log: int, level: int, stream: int, std_dev: float = 0.0):
        """generate_key_switch_key (:367-420) -> (ksk_a [n_in level, dim], ksk_b [n_in level])."""
        r = self.ring
        g = _as_u64(glwe_sk)
        if _is_tensor(lwe_sk):
            ls = lwe_sk.to(torch.int64).contiguous()
        else:
            ls = np.ascontiguousarray(np.asarray(lwe_sk, dtype=np.int64)).view(np.uint64)
        n_in = int(g.numel() if _is_tensor(g) else g.size)
        dim = int(ls.numel() if _is_tensor(ls) else ls.size)
        ka, kb = _empty(g, (n_in * level, dim)), _empty(g, (n_in * level,))
        bg, bl, ba, bb = _Buf(g), _Buf(ls), _Buf(ka, True), _Buf(kb, True)
        w = _where(bg, bl, ba, bb)
        r._bind_stream(w)
        _check(lib().fhe_ksk_generate(r._h, base_log, level, bg.ptr, n_in, bl.ptr, dim, _seed_arr(self.seed), stream,
                                      float(std_dev), ba.ptr, bb.ptr, w))
        return ka, kb

    def pack_key(self, sk, lwe_sk, base_log: int, level: int, stream: int, std_dev: float = 0.0, out=None):
        """The key of EncryptionEngine.pack_lwe (fhe_pack_key_generate): per
        LWE key coefficient i and level l an RLWE encryption (c0, c1) under the
        ring key sk of lwe_sk[i] 2^((level-1-l) base_log) -> PackKey over
        [dim level, 2, n]."""
        r = self.ring
        s = _as_u64(sk.poly if isinstance(sk, SecretKey) else sk)
        if _is_tensor(lwe_sk):
            ls = lwe_sk.to(torch.int64).contiguous()
        else:
            ls = np.ascontiguousarray(np.asarray(lwe_sk, dtype=np.int64)).view(np.uint64)
        dim = int(ls.numel() if _is_tensor(ls) else ls.size)
        out = _empty(s, (dim * level, 2, r.degree)) if out is None else out
        bs, bl, bo = _Buf(s), _Buf(ls), _Buf(out, True)
        if bo.count != dim * level * 2 * r.degree:
            raise FHEError(-9, "pack key must be [dim level, 2, n]")
        w = _where(bs, bl, bo)
        r._bind_stream(w)
        _check(lib().fhe_pack_key_generate(r._h, base_log, level, bs.ptr, bl.ptr, dim, _seed_arr(self.seed), stream,
                                           float(std_dev), bo.ptr, w))
        return PackKey(out, base_log, level, dim)


class PackKey:
    """The packing key-switch key [lwe_dim level, 2, n] with its decomposition
    (KeyGenerator.pack_key; any buffer of that layout serves)."""

    def __init__(self, key, base_log: int, level: int, lwe_dim: int):
        self.key, self.base_log, self.level, self.lwe_dim = key, base_log, level, lwe_dim


def lwe_decrypt(q: int, t: int, sk, lwe_a, lwe_b, device: int = 0):
    """LWE decryption (fhe_lwe_decrypt_batch): (values [batch], phase [batch])."""
    if _is_tensor(lwe_a):
        skv = sk.to(torch.int64).contiguous() if _is_tensor(sk) else torch.as_tensor(np.asarray(sk, dtype=np.int64),
                                                                                      device=lwe_a.device)
    else:
        skv = np.ascontiguousarray(np.asarray(sk, dtype=np.int64)).view(np.uint64)
    a, b = _as_u64(lwe_a), _as_u64(lwe_b)
    batch = int(b.numel() if _is_tensor(b) else b.size)
    dim = int(skv.numel() if _is_tensor(skv) else skv.size)
    vals, ph = _empty(b, (batch,)), _empty(b, (batch,))
    bs, ba, bb, bv, bp = _Buf(skv), _Buf(a), _Buf(b), _Buf(vals, True), _Buf(ph, True)
    w = _where(bs, ba, bb, bv, bp)
    stream = _stream_ptr(bv.device) if w == FHE_DEVICE else None
    _check(lib().fhe_lwe_decrypt_batch(q, t, bs.ptr, dim, ba.ptr, bb.ptr, bv.ptr, bp.ptr, batch, w, device, stream))
    return vals, ph


class DecryptionResult:
    """Batched DecryptionResult (encryption.h): decoded slot values
    [..., n] (slot 0 is decrypt_value's result), the reference's noise budget
    log2(q / (2 max_noise)) per ciphertext, and success = budget >= 0
    (encryption.cpp:289-295)."""

    def __init__(self, values, max_noise, modulus, phase=None):
        import math

        self.values, self.phase = values, phase
        mx = np.asarray(max_noise.cpu() if _is_tensor(max_noise) else max_noise, dtype=np.uint64)
        self.max_noise = mx
        flat = mx.reshape(-1)
        self.noise_budget = np.array([math.log2(float(modulus) / (2.0 * max(float(int(v)), 1.0))) for v in flat])
        self.noise_budget = self.noise_budget.reshape(mx.shape)
        self.success = self.noise_budget >= 0
        self.error = ["" if ok else "Noise budget exhausted - decryption may be incorrect" for ok in
                      self.success.reshape(-1)]


class ScaledMultiplier:
    """The scale-invariant BFV product round(t/q (ct1 (x) ct2)) over the
    integers (fhe_scale_ctx): the result carries Delta m, not the Delta^2 m
    of EncryptionEngine.multiply, and decrypts with real keys after
    relinearisation.  Negacyclic single-device rings only.  Owns the scale
    context (two auxiliary NTT contexts on the ring's device); it borrows
    ``ring`` and keeps it alive."""

    def __init__(self, ring: "PolynomialRing", t: int = 0):
        self._h = None
        h = C.c_void_p()
        _check(lib().fhe_scale_ctx_create(ring._h, int(t), C.byref(h)))
        self._h = h
        self.ring = ring
        info = ScaleInfo()
        _check(lib().fhe_scale_ctx_get_info(h, C.byref(info)))
        self.t, self.aux, self.max_count = int(info.t), (int(info.aux[0]), int(info.aux[1])), int(info.max_count)

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and _lib is not None:
            _lib.fhe_scale_ctx_destroy(h)
        self._h = None

    __del__ = close

    def _run(self, fn, ins, outs, args_of):
        bi = [None if x is None else _Buf(x) for x in ins]
        bo = [_Buf(x, True) for x in outs]
        w = _where(*bi, *bo)
        self.ring._bind_stream(w)
        _check(fn(*args_of([b.ptr if b is not None else None for b in bi], [b.ptr for b in bo], w)))

    def center_lift(self, polys, ref=None):
        """lift(x) mod aux[0], mod aux[1] of rows [..., n] (any u64 words);
        with ref, rows [..., 2, n] of ciphertexts and the lift of ct - ref
        (ref one ciphertext [2, n] for all, or one per ciphertext)."""
        r = self.ring
        polys = _as_u64(polys)
        o1, o2 = _like(polys), _like(polys)
        if ref is None:
            nb = r._batch(polys)
            self._run(lib().fhe_poly_center_lift_batch, [polys], [o1, o2],
                      lambda i, o, w: (self._h, i[0], o[0], o[1], nb, w))
        else:
            nb = _lead(polys, (2, r.degree))
            ref = _as_u64(ref)
            cnt = 1 if tuple(ref.shape) == (2, r.degree) else _lead(ref, (2, r.degree))
            self._run(lib().fhe_ct_center_lift_batch, [polys, ref], [o1, o2],
                      lambda i, o, w: (self._h, i[0], i[1], cnt, o[0], o[1], nb, w))
        return o1, o2

    def scale_round(self, xq, xp1, xp2, out=None):
        """round(t X / q) mod q from X mod q, mod aux[0], mod aux[1], rows [..., n]."""
        xq, xp1, xp2 = _as_u64(xq), _as_u64(xp1), _as_u64(xp2)
        nb = self.ring._batch(xq)
        if tuple(xp1.shape) != tuple(xq.shape) or tuple(xp2.shape) != tuple(xq.shape):
            raise FHEError(-9, "operand shapes differ")
        out = _like(xq) if out is None else out
        self._run(lib().fhe_poly_scale_round_batch, [xq, xp1, xp2], [out],
                  lambda i, o, w: (self._h, i[0], i[1], i[2], o[0], nb, w))
        return out

    def multiply(self, ct1, ct2, out=None):
        """[..., 2, n] x [..., 2, n] -> [..., 3, n]; phase c0 - c1 s + c2 s^2."""
        r = self.ring
        ct1, ct2 = _as_u64(ct1), _as_u64(ct2)
        nb = _lead(ct1, (2, r.degree))
        if tuple(ct2.shape) != tuple(ct1.shape):
            raise FHEError(-9, "ciphertext shapes differ")
        if out is None:
            out = _empty(ct1, tuple(ct1.shape[:-2]) + (3, r.degree))
        self._run(lib().fhe_ct_multiply_scaled_batch, [ct1, ct2], [out],
                  lambda i, o, w: (self._h, i[0], i[1], o[0], nb, w))
        return out

    def dot(self, cts1, cts2, out=None, grouped=None):
        """sum_i cts1[i] (x) cts2[i] with ONE rescale after the sum: [count, 2,
        n] -> [3, n], or [groups, count, 2, n] -> [groups, 3, n].  Not the
        words of a sum of multiply() results (rounding is not linear): one
        rounding error instead of count."""
        r = self.ring
        cts1, cts2 = _as_u64(cts1), _as_u64(cts2)
        shape = tuple(cts1.shape)
        grouped = len(shape) == 4 if grouped is None else bool(grouped)
        lead = 2 if grouped else 1
        if len(shape) != lead + 2 or shape[lead:] != (2, r.degree):
            raise FHEError(-9, "ciphertexts must be [count, 2, n] or [groups, count, 2, n]")
        if tuple(cts2.shape) != shape:
            raise FHEError(-9, "ciphertext shapes differ")
        groups, count = (shape[0], shape[1]) if grouped else (1, shape[0])
        oshape = ((groups,) if grouped else ()) + (3, r.degree)
        if out is None:
            out = _empty(cts1, oshape)
        elif tuple(out.shape) != oshape:
            raise FHEError(-9, f"out must have shape {list(oshape)}")
        self._run(lib().fhe_ct_dot_scaled_batch, [cts1, cts2], [out],
                  lambda i, o, w: (self._h, i[0], i[1], count, groups, o[0], w))
        return out

    def squared_difference(self, cts, expected, out=None):
        """square(cts - expected): expected None, one ciphertext [2, n] for
        all, or one per ciphertext.  The words of multiply(d, d), d = cts - expected."""
        r = self.ring
        cts = _as_u64(cts)
        nb = _lead(cts, (2, r.degree))
        cnt = 0
        if expected is not None:
            expected = _as_u64(expected)
            if tuple(expected.shape) == (2, r.degree):
                cnt = 1
            elif tuple(expected.shape) != tuple(cts.shape):
                raise FHEError(-9, "ciphertext shapes differ")
            else:
                cnt = nb
        if out is None:
            out = _empty(cts, tuple(cts.shape[:-2]) + (3, r.degree))
        self._run(lib().fhe_ct_square_scaled_batch, [cts, expected], [out],
                  lambda i, o, w: (self._h, i[0], i[1], cnt, o[0], nb, w))
        return out

    def square(self, ct, out=None):
        return self.squared_difference(ct, None, out)


def rotation_element(n: int, steps: int, swap: bool = False) -> int:
    """g(steps, swap) = 3^(steps mod n/2) (2n - 1)^swap mod 2n
    (fhe_simd_rotation_element; host arithmetic, no GPU): sigma_g rotates both
    slot rows left by `steps` (negative: right) and swaps them with `swap`."""
    g = C.c_uint32()
    _check(lib().fhe_simd_rotation_element(int(n), int(steps), int(bool(swap)), C.byref(g)))
    return int(g.value)


def slot_sum_elements(n: int):
    """The Galois elements of the slot sum: 3^(2^i) mod 2n for i < log2(n/2),
    then 2n - 1 (log2 n elements)."""
    return [pow(3, 1 << i, 2 * n) for i in range((n // 2).bit_length() - 1)] + [2 * n - 1]


class SimdEncoder:
    """CRT batching (fhe_simd_ctx): n values mod t <-> the plaintext
    polynomial whose evaluations at the 2n-th roots of unity mod t they are,
    so that ring products act slot by slot and the Galois automorphisms
    rotate the slots.  Negacyclic single-device rings, t = 1 mod 2n.  Owns the
    context (an (n, t) transform context and two index tables on the ring's
    device); it borrows ``ring`` and keeps it alive."""

    def __init__(self, ring: "PolynomialRing", t: int):
        self._h = None
        h = C.c_void_p()
        _check(lib().fhe_simd_ctx_create(ring._h, int(t), C.byref(h)))
        self._h = h
        self.ring = ring
        si = SimdInfo()
        _check(lib().fhe_simd_ctx_get_info(h, C.byref(si)))
        self.info = {"q": int(si.q), "t": int(si.t), "psi": int(si.psi), "n": int(si.n), "wordBits": int(si.word_bits)}
        self.t = int(si.t)

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and _lib is not None:
            _lib.fhe_simd_ctx_destroy(h)
        self._h = None

    __del__ = close

    def slot_index(self):
        """k(s): the transform index of slot s, [n] uint32."""
        idx = np.empty(self.ring.degree, dtype=np.uint32)
        _check(lib().fhe_simd_slot_index(self._h, idx.ctypes.data_as(C.POINTER(C.c_uint32))))
        return idx

    def _rows(self, values):
        """[..., n] u64 rows; a short last axis is zero-padded to n (as EncryptionEngine._slots)."""
        n = self.ring.degree
        if _is_tensor(values):
            v = values if values.dim() else values.reshape(1)
            if v.shape[-1] != n:
                pad = torch.zeros(tuple(v.shape[:-1]) + (n,), dtype=v.dtype, device=v.device)
                pad[..., : min(n, v.shape[-1])] = v[..., :n]
                v = pad
            return v.contiguous()
        v = np.asarray(values, dtype=np.uint64)
        v = v.reshape(1) if v.ndim == 0 else v
        if v.shape[-1] != n:
            pad = np.zeros(tuple(v.shape[:-1]) + (n,), dtype=np.uint64)
            pad[..., : min(n, v.shape[-1])] = v[..., :n]
            v = pad
        return np.ascontiguousarray(v)

    def _run(self, fn, x, out, args_of):
        r = self.ring
        nb = r._batch(x)
        out = _like(x) if out is None else out
        bi, bo = _Buf(x), _Buf(out, True)
        if bo.count != bi.count:
            raise FHEError(-9, "output shape differs from the input")
        w = _where(bi, bo)
        r._bind_stream(w)
        _check(fn(*args_of(bi.ptr, bo.ptr, nb, w)))
        return out

    def encode(self, values, lift: bool = False, out=None):
        """Slot values [..., n] (any u64, read mod t; fewer are zero-padded)
        -> plaintext polynomials [..., n] in [0, t); with lift, as centred
        representatives mod q (the form multiply_plain / dot_plain take)."""
        return self._run(lib().fhe_simd_encode_batch, self._rows(values), out,
                         lambda i, o, nb, w: (self._h, i, int(bool(lift)), o, nb, w))

    def decode(self, polys, out=None):
        """Plaintext polynomials [..., n] (any u64, read mod t) -> slot values."""
        return self._run(lib().fhe_simd_decode_batch, _as_u64(polys), out,
                         lambda i, o, nb, w: (self._h, i, o, nb, w))


class EncryptionEngine:
    """Ciphertext arithmetic of EncryptionEngine (encryption.cpp:594-980) over
    batches of ciphertexts [..., 2, n] (c0, c1) / [..., 3, n] (degree 2), and
    encrypt / decrypt / add_plain (:171-348, :638-665) with plaintext modulus
    t (0 selects the reference's default 4, :40-46)."""

    def __init__(self, ring: "PolynomialRing", plaintext_modulus: int = 0):
        self.ring = ring
        self.t = int(plaintext_modulus)
        self.delta = ring.modulus // (self.t or 4)

    def _slots(self, values, nb):
        """Plaintext slot values -> [nb, n] (a scalar or a short vector is
        zero-padded: encode_plaintext / encode_packed, :107-131)."""
        n = self.ring.degree
        if _is_tensor(values):
            v = values.reshape(-1, values.shape[-1]) if values.dim() else values.reshape(1, 1)
            if v.shape[-1] != n:
                pad = torch.zeros((v.shape[0], n), dtype=v.dtype, device=v.device)
                pad[:, : min(n, v.shape[-1])] = v[:, :n]
                v = pad
            if v.shape[0] == 1 and nb > 1:
                v = v.expand(nb, n)
            return v.contiguous()
        v = np.asarray(values, dtype=np.uint64)
        v = v.reshape(1, 1) if v.ndim == 0 else v.reshape(-1, v.shape[-1])
        if v.shape[-1] != n:
            pad = np.zeros((v.shape[0], n), dtype=np.uint64)
            pad[:, : min(n, v.shape[-1])] = v[:, :n]
            v = pad
        if v.shape[0] == 1 and nb > 1:
            v = np.broadcast_to(v, (nb, n))
        return np.ascontiguousarray(v)

    def encrypt(self, values, pk: PublicKey, u, e1, e2, out=None):
        """encrypt_internal (:171-205) with the sampled polynomials supplied:
        u (ternary), e1, e2 (error) [..., n]; values: plaintext slots
        [..., n] (or fewer, zero-padded).  -> ct [..., 2, n]."""
        r = self.ring
        u, e1, e2 = _as_u64(u), _as_u64(e1), _as_u64(e2)
        nb = r._batch(u)
        vals = self._slots(values, nb)
        if out is None:
            out = _empty(u, tuple(u.shape[:-1]) + (2, r.degree))
        bk, bv, bu, b1, b2, bo = _Buf(pk.prep), _Buf(vals), _Buf(u), _Buf(e1), _Buf(e2), _Buf(out, True)
        if not (bv.count == bu.count == b1.count == b2.count == nb * r.degree):
            raise FHEError(-9, "values, u, e1, e2 must all be [batch, n]")
        w = _where(bk, bv, bu, b1, b2, bo)
        r._bind_stream(w)
        _check(lib().fhe_encrypt_batch(r._h, self.t, bk.ptr, bv.ptr, bu.ptr, b1.ptr, b2.ptr, bo.ptr, nb, w))
        return out

    def encrypt_sampled(self, values, pk: PublicKey, seed, stream: int, noise_std: float = 3.2, batch=None,
                        out=None):
        """encrypt_internal (:171-205) with u (ternary), e1, e2 (error) drawn
        on the device from the seeded stream (streams stream .. stream + 2)."""
        r = self.ring
        v = _as_u64(values)
        nb = batch if batch is not None else (r._batch(v) if (v.shape[-1] if len(v.shape) else 0) == r.degree else 1)
        vals = self._slots(values, nb)
        if out is None:
            out = _empty(pk.prep, (nb, 2, r.degree))
        bk, bv, bo = _Buf(pk.prep), _Buf(vals), _Buf(out, True)
        w = _where(bk, bv, bo)
        r._bind_stream(w)
        _check(lib().fhe_encrypt_sampled_batch(r._h, self.t, bk.ptr, bv.ptr, _seed_arr(seed), stream,
                                               float(noise_std), bo.ptr, nb, w))
        return out

    def decrypt(self, ct, sk: SecretKey, is_ntt: bool = False, with_phase: bool = False):
        """decrypt / decrypt_packed (:234-348) for [..., 2, n] or degree-2
        [..., 3, n] ciphertexts -> DecryptionResult."""
        r = self.ring
        ct = _as_u64(ct)
        comps = int(ct.shape[-2]) if len(ct.shape) >= 2 else 0
        if comps not in (2, 3):
            raise FHEError(-9, "ciphertexts must be [..., 2, n] or [..., 3, n]")
        nb = _lead(ct, (comps, r.degree))
        lead = tuple(ct.shape[:-2])
        vals = _empty(ct, lead + (r.degree,))
        mx = _empty(ct, lead if lead else (1,))
        ph = _empty(ct, lead + (r.degree,)) if with_phase else None
        bs, bc, bv, bm = _Buf(sk.prep), _Buf(ct), _Buf(vals, True), _Buf(mx, True)
        bp = _Buf(ph, True) if ph is not None else None
        w = _where(bs, bc, bv, bm, bp)
        r._bind_stream(w)
        _check(lib().fhe_decrypt_batch(r._h, self.t, bs.ptr, bc.ptr, comps, int(bool(is_ntt)), bv.ptr,
                                       bp.ptr if bp else None, bm.ptr, nb, w))
        if _is_tensor(mx):
            torch.cuda.current_stream(mx.device).synchronize()
        return DecryptionResult(vals, mx, r.modulus, ph)

    def partial_decrypt(self, ct, shares, out=None):
        """KeyManager::partial_decrypt (key_manager.cpp:584-601) of every
        ciphertext [..., 2, n] with every given KeyShare, in one launch:
        c1 * share in the ring -> [len(shares), ..., n], or [..., n] for a
        single KeyShare."""
        r = self.ring
        ct = _as_u64(ct)
        single = isinstance(shares, KeyShare)
        lst = [shares] if single else list(shares)
        if not lst:
            raise FHEError(-9, "at least one key share is needed")
        nb = _lead(ct, (2, r.degree))
        lead = tuple(ct.shape[:-2])
        preps = [_placed_like(k.prep, ct) for k in lst]
        prep = preps[0] if len(preps) == 1 else (torch.stack(preps) if _is_tensor(ct) else np.stack(preps))
        shape = (() if single else (len(lst),)) + lead + (r.degree,)
        if out is None:
            out = _empty(ct, shape)
        bs, bc, bo = _Buf(prep), _Buf(ct), _Buf(out, True)
        if bo.count != len(lst) * nb * r.degree:
            raise FHEError(-9, f"out must have shape {list(shape)}")
        w = _where(bs, bc, bo)
        r._bind_stream(w)
        _check(lib().fhe_partial_decrypt_batch(r._h, bs.ptr, len(lst), bc.ptr, bo.ptr, nb, w))
        return out

    def combine_partial_decryptions(self, ct, partials, share_ids, threshold=None, with_phase: bool = False):
        """KeyManager::combine_partial_decryptions (key_manager.cpp:604-636)
        and the decryption it opens: partials [count, ..., n] (an array, or a
        list of [..., n] blocks, one per trustee) for the ciphertexts
        [..., 2, n], share_ids their ids.  As the reference, the Lagrange
        coefficients interpolate over every id given and the first
        ``threshold`` partials (default: all) are summed; phase = c0 - sum,
        decoded like decrypt -> DecryptionResult (with max_noise)."""
        r = self.ring
        ct = _as_u64(ct)
        ids = [int(i) for i in share_ids]
        threshold = len(ids) if threshold is None else int(threshold)
        if isinstance(partials, (list, tuple)):
            blocks = [_placed_like(_as_u64(p), ct) for p in partials]
            partials = (torch.stack(blocks) if _is_tensor(ct) else np.stack(blocks)) if blocks else None
        else:
            partials = _placed_like(_as_u64(partials), ct)
        count = 0 if partials is None else int(partials.shape[0])
        if count != len(ids):
            raise FHEError(-9, "one share id per partial decryption is needed")
        if count < threshold or threshold < 1:
            raise FHEError(-9, "Not enough partial decryptions")
        return self.combine_partials(ct, partials[:threshold], lagrange_coefficients(r.modulus, ids, threshold), with_phase)

    def combine_partials(self, ct, partials, lambdas, with_phase: bool = False):
        """phase = c0 - sum_i partials[i] lambdas[i] for ct [..., 2, n] and
        partials [count, ..., n], decoded like decrypt (fhe_combine_partials_batch)
        -> DecryptionResult.  lambdas: count integers (any u64, read mod q)."""
        r = self.ring
        ct = _as_u64(ct)
        partials = _placed_like(_as_u64(partials), ct)
        lam = [int(x) for x in lambdas]
        nb = _lead(ct, (2, r.degree))
        lead = tuple(ct.shape[:-2])
        if not lam or tuple(partials.shape) != (len(lam),) + lead + (r.degree,):
            raise FHEError(-9, f"partials must have shape {[len(lam)] + list(lead) + [r.degree]}, one block per lambda")
        vals = _empty(ct, lead + (r.degree,))
        mx = _empty(ct, lead if lead else (1,))
        ph = _empty(ct, lead + (r.degree,)) if with_phase else None
        bc, bq, bv, bm = _Buf(ct), _Buf(partials), _Buf(vals, True), _Buf(mx, True)
        bp = _Buf(ph, True) if ph is not None else None
        w = _where(bc, bq, bv, bm, bp)
        r._bind_stream(w)
        _check(lib().fhe_combine_partials_batch(r._h, self.t, bc.ptr, bq.ptr, (C.c_uint64 * len(lam))(*lam), len(lam),
                                                bv.ptr, bp.ptr if bp else None, bm.ptr, nb, w))
        if _is_tensor(mx):
            torch.cuda.current_stream(mx.device).synchronize()
        return DecryptionResult(vals, mx, r.modulus, ph)

    def decrypt_value(self, ct, sk: SecretKey, is_ntt: bool = False):
        """decrypt_value (:303-310): slot 0, or None where decryption failed."""
        res = self.decrypt(ct, sk, is_ntt)
        v = res.values.cpu().numpy().view(np.uint64) if _is_tensor(res.values) else res.values
        return [int(x) if ok else None for x, ok in zip(v.reshape(-1, self.ring.degree)[:, 0], res.success.reshape(-1))]

    def add_plain(self, ct, values, is_ntt: bool = False, out=None):
        """add_plain (:638-665): (c0 + encode(values), c1)."""
        r = self.ring
        ct = _as_u64(ct)
        nb = _lead(ct, (2, r.degree))
        vals = self._slots(values, nb)
        out = _like(ct) if out is None else out
        bc, bv, bo = _Buf(ct), _Buf(vals), _Buf(out, True)
        w = _where(bc, bv, bo)
        r._bind_stream(w)
        _check(lib().fhe_add_plain_batch(r._h, self.t, bc.ptr, bv.ptr, int(bool(is_ntt)), bo.ptr, nb, w))
        return out

    def _pair(self, ct1, ct2):
        ct1, ct2 = _as_u64(ct1), _as_u64(ct2)
        _lead(ct1, (2, self.ring.degree))
        if tuple(ct2.shape) != tuple(ct1.shape):
            raise FHEError(-9, "ciphertext shapes differ")
        return ct1, ct2

    def add(self, ct1, ct2, out=None):
        """add (:594-617): componentwise mod_add of (c0, c1)."""
        ct1, ct2 = self._pair(ct1, ct2)
        return self.ring.add(ct1, ct2, out)

    def batch_add(self, cts, out=None):
        """batch_add / batch_add_tree (:1327-1460): the sum of the ciphertexts
        cts [count, 2 | 3, n] (or a list of them; a list of device tensors is
        summed in place, no copy) -> [2 | 3, n], in one launch."""
        r = self.ring
        if isinstance(cts, (list, tuple)):
            if len(cts) == 0:
                raise FHEError(-9, "Cannot add empty vector of ciphertexts")
            if all(_is_tensor(c) for c in cts):
                for c in cts:
                    if len(c.shape) != 2 or c.shape[0] not in (2, 3):
                        raise FHEError(-9, "ciphertexts must be [2, n] or [3, n]")
                return r.sum_buffers(cts, out)
            cts = np.stack([np.asarray(c, dtype=np.uint64) for c in cts])
        cts = _as_u64(cts)
        if len(cts.shape) != 3 or cts.shape[1] not in (2, 3):
            raise FHEError(-9, "ciphertexts must be [count, 2, n] or [count, 3, n]")
        return r.sum_batch(cts, out, grouped=False)

    tally_votes = batch_add  # tally_votes (:1061-1067) is batch_add_tree

    def tally_multi_candidate(self, cts, num_candidates: int, out=None):
        """tally_multi_candidate (:1153-1168): packed ballots, one slot per
        candidate; the sum keeps the slots."""
        if num_candidates > self.ring.degree:
            raise FHEError(-9, "Number of candidates exceeds polynomial degree")
        return self.batch_add(cts, out)

    def dot(self, cts1, cts2, is_ntt: bool = False, out=None, accumulate: bool = False, grouped=None):
        """Ciphertext inner product in one fused launch: the degree-2 sum
        sum_i multiply(cts1[i], cts2[i]) folded by add(), with no intermediate
        ciphertexts.  cts [count, 2, n] -> [3, n], or [groups, count, 2, n] ->
        [groups, 3, n]; grouped=None reads a 4-d input as grouped.  Words equal
        multiply() followed by batch_add().  accumulate: `out` is one more
        degree-2 term of each sum."""
        r = self.ring
        cts1, cts2 = _as_u64(cts1), _as_u64(cts2)
        shape = tuple(cts1.shape)
        grouped = len(shape) == 4 if grouped is None else bool(grouped)
        lead = 2 if grouped else 1
        if len(shape) != lead + 2 or shape[lead:] != (2, r.degree):
            raise FHEError(-9, "ciphertexts must be [count, 2, n] or [groups, count, 2, n]")
        if tuple(cts2.shape) != shape:
            raise FHEError(-9, "ciphertext shapes differ")
        groups, count = (shape[0], shape[1]) if grouped else (1, shape[0])
        if count == 0:
            raise FHEError(-9, "Cannot tally empty ballot list")
        oshape = ((groups,) if grouped else ()) + (3, r.degree)
        if out is None:
            if accumulate:
                raise FHEError(-9, "accumulate needs an out buffer")
            out = _empty(cts1, oshape)
        elif tuple(out.shape) != oshape:
            raise FHEError(-9, f"out must have shape {list(oshape)}")
        b1, b2, bo = _Buf(cts1), _Buf(cts2), _Buf(out, True)
        w = _where(b1, b2, bo)
        r._bind_stream(w)
        _check(lib().fhe_ct_dot_batch(r._h, b1.ptr, b2.ptr, count, groups, int(bool(is_ntt)), int(bool(accumulate)),
                                      bo.ptr, w))
        return out

    def dot_buffers(self, bufs1, bufs2, is_ntt: bool = False, out=None, accumulate: bool = False):
        """dot over separately allocated device ciphertexts [2, n]; a tensor
        may be listed twice, and bufs1[i] is bufs2[i] gives a square."""
        r = self.ring
        bufs1, bufs2 = list(bufs1), list(bufs2)
        if len(bufs1) != len(bufs2):
            raise FHEError(-9, "Ballots and weights must have the same size")
        if not bufs1:
            raise FHEError(-9, "Cannot tally empty ballot list")
        if any(tuple(b.shape) != (2, r.degree) for b in bufs1 + bufs2):
            raise FHEError(-9, "ciphertexts must be [2, n]")
        if out is None:
            if accumulate:
                raise FHEError(-9, "accumulate needs an out buffer")
            out = torch.empty((3, r.degree), dtype=bufs1[0].dtype, device=bufs1[0].device)
        elif tuple(out.shape) != (3, r.degree):
            raise FHEError(-9, f"out must have shape {[3, r.degree]}")
        b1, b2, bo = [_Buf(b) for b in bufs1], [_Buf(b) for b in bufs2], _Buf(out, True)
        if _where(bo, *b1, *b2) != FHE_DEVICE:
            raise FHEError(-9, "dot_buffers takes device tensors (stack host arrays for dot)")
        r._bind_stream(FHE_DEVICE)
        t1 = (C.c_void_p * len(b1))(*[b.ptr for b in b1])
        t2 = (C.c_void_p * len(b2))(*[b.ptr for b in b2])
        _check(lib().fhe_ct_dot_ptrs(r._h, t1, t2, len(b1), int(bool(is_ntt)), int(bool(accumulate)), bo.ptr))
        return out

    def tally_scalar_weighted(self, cts, scalars, out=None):
        """Public integer weights: sum_i multiply_scalar(cts[i], scalars[i])
        folded by add(), in one launch.  cts [count, 2 | 3, n] (or a list of
        them; a list of device tensors is read in place), scalars `count`
        integers -> [2 | 3, n]."""
        r = self.ring
        if len(cts) != len(scalars):
            raise FHEError(-9, "Ballots and weights must have the same size")
        if isinstance(cts, (list, tuple)):
            if len(cts) == 0:
                raise FHEError(-9, "Cannot add empty vector of ciphertexts")
            if all(_is_tensor(c) for c in cts):
                for c in cts:
                    if len(c.shape) != 2 or c.shape[0] not in (2, 3):
                        raise FHEError(-9, "ciphertexts must be [2, n] or [3, n]")
                return r.sum_scaled_buffers(cts, scalars, out)
            cts = np.stack([np.asarray(c, dtype=np.uint64) for c in cts])
        cts = _as_u64(cts)
        if len(cts.shape) != 3 or cts.shape[1] not in (2, 3):
            raise FHEError(-9, "ciphertexts must be [count, 2, n] or [count, 3, n]")
        if not _is_tensor(scalars):
            scalars = np.asarray([int(s) & (2**64 - 1) for s in scalars], dtype=np.uint64)
        return r.sum_scaled(cts, scalars, out, grouped=False)

    def dot_plain(self, cts, pts, is_ntt: bool = False, out=None, accumulate: bool = False, grouped=None):
        """Public plaintext-polynomial weights in one fused launch: the
        degree-1 sum sum_i multiply_plain(cts[i], pts[i]) folded by add(), with
        no intermediate ciphertexts.  cts [count, 2, n] and already-encoded
        pts [count, n] -> [2, n], or [groups, count, 2, n] and
        [groups, count, n] -> [groups, 2, n]; grouped=None reads a 4-d cts as
        grouped.  is_ntt: cts and the result are NTT-domain, pts are still
        coefficient form.  Words equal multiply_plain() followed by
        batch_add().  accumulate: `out` is one more degree-1 term."""
        r = self.ring
        cts, pts = _as_u64(cts), _as_u64(pts)
        shape = tuple(cts.shape)
        grouped = len(shape) == 4 if grouped is None else bool(grouped)
        lead = 2 if grouped else 1
        if len(shape) != lead + 2 or shape[lead:] != (2, r.degree):
            raise FHEError(-9, "ciphertexts must be [count, 2, n] or [groups, count, 2, n]")
        if tuple(pts.shape) != shape[:lead] + (r.degree,):
            raise FHEError(-9, "plaintexts must be [count, n] or [groups, count, n]")
        groups, count = (shape[0], shape[1]) if grouped else (1, shape[0])
        if count == 0:
            raise FHEError(-9, "Cannot tally empty ballot list")
        oshape = ((groups,) if grouped else ()) + (2, r.degree)
        if out is None:
            if accumulate:
                raise FHEError(-9, "accumulate needs an out buffer")
            out = _empty(cts, oshape)
        elif tuple(out.shape) != oshape:
            raise FHEError(-9, f"out must have shape {list(oshape)}")
        b1, b2, bo = _Buf(cts), _Buf(pts), _Buf(out, True)
        w = _where(b1, b2, bo)
        r._bind_stream(w)
        _check(lib().fhe_ct_dot_plain_batch(r._h, b1.ptr, b2.ptr, count, groups, int(bool(is_ntt)),
                                            int(bool(accumulate)), bo.ptr, w))
        return out

    def dot_plain_buffers(self, bufs, pts, is_ntt: bool = False, out=None, accumulate: bool = False):
        """dot_plain over separately allocated device ciphertexts [2, n] and
        plaintext polynomials [n]; a tensor may be listed twice (one plaintext
        may weigh several ballots)."""
        r = self.ring
        bufs, pts = list(bufs), list(pts)
        if len(bufs) != len(pts):
            raise FHEError(-9, "Ballots and weights must have the same size")
        if not bufs:
            raise FHEError(-9, "Cannot tally empty ballot list")
        if any(tuple(b.shape) != (2, r.degree) for b in bufs):
            raise FHEError(-9, "ciphertexts must be [2, n]")
        if any(tuple(p.shape) != (r.degree,) for p in pts):
            raise FHEError(-9, "plaintexts must be [n]")
        if out is None:
            if accumulate:
                raise FHEError(-9, "accumulate needs an out buffer")
            out = torch.empty((2, r.degree), dtype=bufs[0].dtype, device=bufs[0].device)
        elif tuple(out.shape) != (2, r.degree):
            raise FHEError(-9, f"out must have shape {[2, r.degree]}")
        b1, b2, bo = [_Buf(b) for b in bufs], [_Buf(p) for p in pts], _Buf(out, True)
        if _where(bo, *b1, *b2) != FHE_DEVICE:
            raise FHEError(-9, "dot_plain_buffers takes device tensors (stack host arrays for dot_plain)")
        r._bind_stream(FHE_DEVICE)
        t1 = (C.c_void_p * len(b1))(*[b.ptr for b in b1])
        t2 = (C.c_void_p * len(b2))(*[b.ptr for b in b2])
        _check(lib().fhe_ct_dot_plain_ptrs(r._h, t1, t2, len(b1), int(bool(is_ntt)), int(bool(accumulate)), bo.ptr))
        return out

    def tally_weighted_votes(self, ballots, weights, ek: EvaluationKey, relinearize: str = "each", out=None):
        """tally_weighted_votes (:1069-1110): sum_i ballots[i] * weights[i] as
        a degree-1 ciphertext [2, n].  relinearize="each" is the reference's
        multiply_relin per ballot followed by batch_add (its words);
        relinearize="once" is dot() followed by one relinearisation: the same
        plaintext with less noise, not the same words (the digit decomposition
        is not linear)."""
        if relinearize not in ("each", "once"):
            raise FHEError(-9, "relinearize must be 'each' or 'once'")
        if len(ballots) != len(weights):
            raise FHEError(-9, "Ballots and weights must have the same size")
        if len(ballots) == 0:
            raise FHEError(-9, "Cannot tally empty ballot list")
        lists = isinstance(ballots, (list, tuple)) and isinstance(weights, (list, tuple))
        if lists and all(_is_tensor(c) for c in list(ballots) + list(weights)):
            if relinearize == "once":
                return self.relinearize(self.dot_buffers(ballots, weights), ek, out)
            ballots, weights = torch.stack(list(ballots)), torch.stack(list(weights))
        if isinstance(ballots, (list, tuple)):
            ballots = np.stack([np.asarray(c, dtype=np.uint64) for c in ballots])
        if isinstance(weights, (list, tuple)):
            weights = np.stack([np.asarray(c, dtype=np.uint64) for c in weights])
        if relinearize == "once":
            return self.relinearize(self.dot(ballots, weights, grouped=False), ek, out)
        return self.batch_add(self.multiply_relin(ballots, weights, ek), out)

    def subtract(self, ct1, ct2, out=None):
        """subtract (:692-714)."""
        ct1, ct2 = self._pair(ct1, ct2)
        return self.ring.subtract(ct1, ct2, out)

    def negate(self, ct, out=None):
        """negate (:716-727)."""
        ct = _as_u64(ct)
        _lead(ct, (2, self.ring.degree))
        return self.ring.negate(ct, out)

    def multiply_scalar(self, ct, scalar: int, out=None):
        """multiply_scalar (:890-902)."""
        ct = _as_u64(ct)
        _lead(ct, (2, self.ring.degree))
        return self.ring.multiply_scalar(ct, scalar, out)

    def multiply_plain(self, ct, pt, out=None):
        """multiply_plain (:809-850) for an already-encoded plaintext
        polynomial pt [..., n] (one per ciphertext, or one for all): each
        component times pt through the fused polymul (coefficient form)."""
        r = self.ring
        ct = _as_u64(ct)
        nb = _lead(ct, (2, r.degree))
        pt = _as_u64(pt)
        if _is_tensor(ct):
            ptb = pt.reshape(-1, 1, r.degree).expand(nb, 2, r.degree).reshape(ct.shape).contiguous()
        else:
            ptb = np.ascontiguousarray(np.broadcast_to(np.asarray(pt).reshape(-1, 1, r.degree),
                                                       (nb, 2, r.degree)).reshape(ct.shape))
        return r.multiply(ct, ptb, out)

    def multiply(self, ct1, ct2, is_ntt: bool = False, out=None):
        """multiply (:737-798): tensor product -> [..., 3, n]."""
        r = self.ring
        ct1, ct2 = _as_u64(ct1), _as_u64(ct2)
        nb = _lead(ct1, (2, r.degree))
        if tuple(ct2.shape) != tuple(ct1.shape):
            raise FHEError(-9, "ciphertext shapes differ")
        if out is None:
            out = _empty(ct1, tuple(ct1.shape[:-2]) + (3, r.degree))
        b1, b2, bo = _Buf(ct1), _Buf(ct2), _Buf(out, True)
        w = _where(b1, b2, bo)
        r._bind_stream(w)
        _check(lib().fhe_ct_multiply_batch(r._h, b1.ptr, b2.ptr, bo.ptr, nb, int(bool(is_ntt)), w))
        return out

    def relinearize(self, ct3, ek: EvaluationKey, out=None):
        """relinearize (:904-980): [..., 3, n] -> [..., 2, n]; a degree-1
        input [..., 2, n] is returned as a copy (:906-909)."""
        r = self.ring
        ct3 = _as_u64(ct3)
        if len(ct3.shape) >= 2 and tuple(ct3.shape[-2:]) == (2, r.degree):
            if out is None:
                return ct3.clone() if _is_tensor(ct3) else ct3.copy()
            out[...] = ct3
            return out
        nb = _lead(ct3, (3, r.degree))
        if out is None:
            out = _empty(ct3, tuple(ct3.shape[:-2]) + (2, r.degree))
        bi, bk, bo = _Buf(ct3), _Buf(ek.rlk_ntt), _Buf(out, True)
        w = _where(bi, bo) if not ek.level else _where(bi, bk, bo)
        r._bind_stream(w)
        _check(lib().fhe_relinearize_batch(r._h, ek.decomp_base_log, ek.level, bi.ptr, bk.ptr if ek.level else None,
                                           bo.ptr, nb, w))
        return out

    def multiply_relin(self, ct1, ct2, ek: EvaluationKey, out=None):
        """multiply_relin (:800-807)."""
        r = self.ring
        ct1, ct2 = _as_u64(ct1), _as_u64(ct2)
        nb = _lead(ct1, (2, r.degree))
        if tuple(ct2.shape) != tuple(ct1.shape):
            raise FHEError(-9, "ciphertext shapes differ")
        out = _like(ct1) if out is None else out
        b1, b2, bk, bo = _Buf(ct1), _Buf(ct2), _Buf(ek.rlk_ntt), _Buf(out, True)
        w = _where(b1, b2, bo) if not ek.level else _where(b1, b2, bk, bo)
        r._bind_stream(w)
        _check(lib().fhe_ct_multiply_relin_batch(r._h, ek.decomp_base_log, ek.level, b1.ptr, b2.ptr,
                                                 bk.ptr if ek.level else None, bo.ptr, nb, w))
        return out

    def _expected(self, cts, expected):
        """(buffer, ref_count) of the `expected` argument of the squaring
        methods: None, one ciphertext [2, n] for all, or the shape of cts."""
        if expected is None:
            return None, 0
        expected = _as_u64(expected)
        if tuple(expected.shape) == (2, self.ring.degree):
            return _Buf(expected), 1
        if tuple(expected.shape) != tuple(cts.shape):
            raise FHEError(-9, "ciphertext shapes differ")
        return _Buf(expected), _lead(cts, (2, self.ring.degree))

    def squared_difference(self, cts, expected, is_ntt: bool = False, out=None):
        """square(subtract(ct, expected)) (:1004-1035 after :692-714) in one
        kernel -> [..., 3, n]; expected is one ciphertext [2, n] shared by all
        of cts, or one per ciphertext (the shape of cts).  The words equal
        multiply(d, d) of d = subtract(cts, expected)."""
        r = self.ring
        cts = _as_u64(cts)
        nb = _lead(cts, (2, r.degree))
        be, cnt = self._expected(cts, expected)
        if out is None:
            out = _empty(cts, tuple(cts.shape[:-2]) + (3, r.degree))
        bc, bo = _Buf(cts), _Buf(out, True)
        w = _where(bc, be, bo)
        r._bind_stream(w)
        _check(lib().fhe_ct_square_batch(r._h, bc.ptr, be.ptr if be else None, cnt, bo.ptr, nb, int(bool(is_ntt)), w))
        return out

    def square(self, ct, is_ntt: bool = False, out=None):
        """square (:1004-1035): 2 forward + 3 inverse transforms -> [..., 3, n]."""
        return self.squared_difference(ct, None, is_ntt, out)

    def compute_anomaly_score(self, cts, expected, ek: EvaluationKey, out=None):
        """compute_anomaly_score (:1305-1321): relinearize(square(subtract(ct,
        expected))) -> [..., 2, n]; expected as in squared_difference."""
        r = self.ring
        cts = _as_u64(cts)
        nb = _lead(cts, (2, r.degree))
        be, cnt = self._expected(cts, expected)
        out = _like(cts) if out is None else out
        bc, bk, bo = _Buf(cts), _Buf(ek.rlk_ntt), _Buf(out, True)
        w = _where(bc, be, bo) if not ek.level else _where(bc, be, bk, bo)
        r._bind_stream(w)
        _check(lib().fhe_ct_square_relin_batch(r._h, ek.decomp_base_log, ek.level, bc.ptr, be.ptr if be else None, cnt,
                                               bk.ptr if ek.level else None, bo.ptr, nb, w))
        return out

    def square_relin(self, ct, ek: EvaluationKey, out=None):
        """square_relin (:1037-1055)."""
        return self.compute_anomaly_score(ct, None, ek, out)

    # -- scale-invariant products (ScaledMultiplier with this engine's t): results carry Delta m and
    # decrypt with real keys after relinearize(); negacyclic rings only
    @property
    def scaled(self) -> "ScaledMultiplier":
        if getattr(self, "_scaled", None) is None:
            self._scaled = ScaledMultiplier(self.ring, self.t)
        return self._scaled

    def multiply_scaled(self, ct1, ct2, out=None):
        """round(t/q (ct1 (x) ct2)) -> [..., 3, n] (ScaledMultiplier.multiply)."""
        return self.scaled.multiply(ct1, ct2, out)

    def dot_scaled(self, cts1, cts2, out=None, grouped=None):
        """Inner product with one rescale after the sum (ScaledMultiplier.dot)."""
        return self.scaled.dot(cts1, cts2, out, grouped)

    def square_scaled(self, ct, out=None):
        return self.scaled.squared_difference(ct, None, out)

    def squared_difference_scaled(self, cts, expected, out=None):
        return self.scaled.squared_difference(cts, expected, out)

    def multiply_relin_scaled(self, ct1, ct2, ek: EvaluationKey, out=None):
        """relinearize(multiply_scaled(ct1, ct2)) -> [..., 2, n]."""
        return self.relinearize(self.multiply_scaled(ct1, ct2), ek, out)

    def tally_weighted_votes_scaled(self, ballots, weights, ek: EvaluationKey, out=None):
        """sum_i ballots[i] * weights[i] under encrypted weights as a degree-1
        ciphertext [2, n] that decrypts with real keys: dot_scaled, then one
        relinearisation."""
        if len(ballots) != len(weights):
            raise FHEError(-9, "Ballots and weights must have the same size")
        if len(ballots) == 0:
            raise FHEError(-9, "Cannot tally empty ballot list")
        stack = lambda x: (torch.stack(list(x)) if all(_is_tensor(c) for c in x)
                           else np.stack([np.asarray(c, dtype=np.uint64) for c in x]))
        if isinstance(ballots, (list, tuple)):
            ballots = stack(ballots)
        if isinstance(weights, (list, tuple)):
            weights = stack(weights)
        return self.relinearize(self.dot_scaled(ballots, weights, grouped=False), ek, out)

    def pack_lwe(self, lwe_a, lwe_b, slots, pack_key: "PackKey", out=None, accumulate: bool = False):
        """The packing key switch (fhe_lwe_pack_batch): LWE ciphertexts
        (a [..., S, dim], b [..., S]) -- the pair every Comparisons method
        returns -- become one BFV ciphertext [..., 2, n] per leading index
        whose phase has LWE s's message at coefficient slots[s] (slots may
        repeat: the messages add).  accumulate adds to `out`.  Slots other than
        0 need the negacyclic mode to decrypt."""
        r = self.ring
        lwe_a, lwe_b = _as_u64(lwe_a), _as_u64(lwe_b)
        slots = [int(s) for s in slots]
        S, dim = len(slots), pack_key.lwe_dim
        if any(s < 0 or s >= 1 << 32 for s in slots):
            raise FHEError(-9, "slot index out of range")
        if len(lwe_a.shape) < 2 or tuple(lwe_a.shape[-2:]) != (S, dim) or tuple(lwe_a.shape[:-1]) != tuple(lwe_b.shape):
            raise FHEError(-9, "LWE masks must be [..., S, dim] and bodies [..., S]")
        lead = tuple(lwe_b.shape[:-1])
        if out is None:
            if accumulate:
                raise FHEError(-9, "accumulate needs an output to add to")
            out = _empty(lwe_a, lead + (2, r.degree))
        bk, ba, bb, bo = _Buf(_as_u64(pack_key.key)), _Buf(lwe_a), _Buf(lwe_b), _Buf(out, True)
        nb = bb.count // S if S else 0
        if bo.count != nb * 2 * r.degree or bk.count != dim * pack_key.level * 2 * r.degree:
            raise FHEError(-9, "output must be [..., 2, n] and the key [dim level, 2, n]")
        w = _where(bk, ba, bb, bo)
        r._bind_stream(w)
        _check(lib().fhe_lwe_pack_batch(r._h, pack_key.base_log, pack_key.level, dim, bk.ptr, ba.ptr, bb.ptr,
                                        (C.c_uint32 * max(1, S))(*slots), S, int(bool(accumulate)), bo.ptr, nb, w))
        return out


    def apply_galois(self, ct, key: "SwitchKey", add_input: bool = False, out=None):
        """fhe_ct_galois_batch: [..., 2, n] -> the encryption under the key's
        target of sigma_g of the message (g = key.g), plus ct itself with
        add_input.  g != 1 needs the negacyclic mode to decrypt."""
        r = self.ring
        if key.steps is not None:
            raise FHEError(-9, "apply_galois takes one key [level, 2, n]")
        ct = _as_u64(ct)
        nb = _lead(ct, (2, r.degree))
        out = _like(ct) if out is None else out
        bi, bo = _Buf(ct), _Buf(out, True)
        bk = _Buf(key.key_ntt) if key.level else None
        w = _where(bi, bk, bo)
        r._bind_stream(w)
        _check(lib().fhe_ct_galois_batch(r._h, key.base_log, key.level, int(key.g), bk.ptr if bk else None, bi.ptr,
                                         int(bool(add_input)), bo.ptr, nb, w))
        return out

    def rekey(self, ct, key: "SwitchKey", out=None):
        """Hands a ciphertext to another secret key without decrypting it: a
        key switch with a re-keying key (KeyGenerator.switch_key with g = 1)."""
        if key.steps is not None or key.g != 1:
            raise FHEError(-9, "rekey needs a key with g = 1")
        return self.apply_galois(ct, key, False, out)

    def trace(self, ct, keys: "SwitchKey", steps=None, out=None):
        """fhe_ct_trace_batch: after `steps` automorphism steps (default: all
        of keys) only the coefficients of the phase at multiples of 2^steps
        remain, exactly; the rest become key-switch noise around 0."""
        r = self.ring
        if keys.steps is None:
            raise FHEError(-9, "trace needs the keys of KeyGenerator.galois_keys [steps, level, 2, n]")
        steps = keys.steps if steps is None else int(steps)
        if steps < 1 or steps > keys.steps:
            raise FHEError(-9, "steps must be between 1 and the number of keys")
        ct = _as_u64(ct)
        nb = _lead(ct, (2, r.degree))
        out = _like(ct) if out is None else out
        bi, bo = _Buf(ct), _Buf(out, True)
        bk = _Buf(keys.key_ntt) if keys.level else None
        w = _where(bi, bk, bo)
        r._bind_stream(w)
        _check(lib().fhe_ct_trace_batch(r._h, keys.base_log, keys.level, steps, bk.ptr if bk else None, bi.ptr,
                                        bo.ptr, nb, w))
        return out

    def isolate_slot(self, ct, slot: int, keys: "SwitchKey", out=None):
        """Zeroes every coefficient of the message but `slot`: rotate by
        X^-slot, the full trace, rotate back by X^+slot.  Needs the log2(n)
        keys of KeyGenerator.galois_keys and the negacyclic mode."""
        r = self.ring
        if keys.steps != r.degree.bit_length() - 1:
            raise FHEError(-9, "isolate_slot needs the log2(n) keys of the full trace")
        slot = int(slot)
        if slot < 0 or slot >= r.degree:
            raise FHEError(-9, "slot index out of range")
        ct = _as_u64(ct)
        nb = _lead(ct, (2, r.degree))
        rot = BootstrapEngine(r, keys.base_log, max(1, keys.level))
        x = rot.multiply_glwe_by_monomial(ct, [-slot] * nb)
        y = self.trace(x, keys)
        return rot.multiply_glwe_by_monomial(y, [slot] * nb, out=x if out is None else out)

    # -- SIMD batching (SimdEncoder with this engine's t): slot-wise products, slot rotations and slot
    # sums.  These are SIMD slots; isolate_slot / slot_extract / pack_lwe address coefficients.
    @property
    def simd(self) -> "SimdEncoder":
        if getattr(self, "_simd", None) is None:
            self._simd = SimdEncoder(self.ring, self.t or 4)
        return self._simd

    def encode_simd(self, values, lift: bool = False, out=None):
        """Slot values -> the plaintext polynomial encrypt() / add_plain() take as `values`."""
        return self.simd.encode(values, lift, out)

    def decode_simd(self, polys, out=None):
        return self.simd.decode(polys, out)

    def decrypt_simd(self, ct, sk: SecretKey):
        """decrypt, then decode: a DecryptionResult whose values are the slot values."""
        res = self.decrypt(ct, sk)
        res.values = self.simd.decode(res.values)
        return res

    def galois_chain(self, ct, gs, keys: "SwitchKey", key_idx=None, add_input: bool = False, out=None):
        """fhe_ct_galois_chain_batch: x <- apply_galois(gs[i], key key_idx[i]
        (default i) of `keys` [nkeys, level, 2, n], x, add_input) for every i in
        one call, word for word that chain of calls."""
        r = self.ring
        if keys.steps is None:
            raise FHEError(-9, "galois_chain needs keys [nkeys, level, 2, n]")
        gs = [int(g) for g in gs]
        idx = list(range(len(gs))) if key_idx is None else [int(k) for k in key_idx]
        if len(idx) != len(gs):
            raise FHEError(-9, "gs and key_idx must have the same length")
        if any(k < 0 or k >= keys.steps for k in idx):
            raise FHEError(-9, "key index out of range")
        if any(g < 0 or g >= 1 << 32 for g in gs):
            raise FHEError(-9, "Galois element out of range")
        ct = _as_u64(ct)
        nb = _lead(ct, (2, r.degree))
        out = _like(ct) if out is None else out
        bi, bo = _Buf(ct), _Buf(out, True)
        bk = _Buf(keys.key_ntt) if keys.level else None
        w = _where(bi, bk, bo)
        r._bind_stream(w)
        ns = len(gs)
        _check(lib().fhe_ct_galois_chain_batch(r._h, keys.base_log, keys.level, ns, (C.c_uint32 * max(1, ns))(*gs),
                                               (C.c_uint32 * max(1, ns))(*idx), bk.ptr if bk else None, bi.ptr,
                                               int(bool(add_input)), bo.ptr, nb, w))
        return out

    def _rotation_keys(self, keys):
        n = self.ring.degree
        if keys.steps is None or list(keys.g) != slot_sum_elements(n):
            raise FHEError(-9, "needs the keys of KeyGenerator.rotation_keys")

    def rotate_rows(self, ct, steps: int, keys: "SwitchKey", out=None):
        """Both slot rows rotated left by `steps` (negative: right): the
        binary decomposition of steps mod n/2 over the power-of-two keys, one
        chain call.  A multiple of n/2 copies the reduced words."""
        self._rotation_keys(keys)
        n = self.ring.degree
        m = int(steps) % (n // 2)
        bits = [i for i in range((n // 2).bit_length() - 1) if (m >> i) & 1]
        if not bits:
            return self.ring.galois(_as_u64(ct), 1, out)
        return self.galois_chain(ct, [keys.g[i] for i in bits], keys, bits, False, out)

    def rotate_columns(self, ct, keys: "SwitchKey", out=None):
        """The two slot rows swapped (sigma_{2n-1})."""
        self._rotation_keys(keys)
        last = keys.steps - 1
        return self.galois_chain(ct, [keys.g[last]], keys, [last], False, out)

    def sum_slots(self, ct, keys: "SwitchKey", rows_only: bool = False, out=None):
        """sum_s v_s in every slot (rows_only: each slot its row's sum):
        x <- x + sigma_g(x) over the keys.  Every step doubles the noise and
        adds one key switch; see include/fhe_gpu.h for the limit at t = 65537."""
        self._rotation_keys(keys)
        ns = keys.steps - 1 if rows_only else keys.steps
        if ns == 0:
            return self.ring.galois(_as_u64(ct), 1, out)
        return self.galois_chain(ct, list(keys.g[:ns]), keys, None, True, out)

    # ---- hoisted rotations and the plaintext linear transform
    def hoist(self, ct, base_log: int, level: int, out=None) -> "HoistedCiphertext":
        """fhe_ct_hoist_batch: decompose and transform ct [..., 2, n] once for
        any number of rotations with keys of the same (base_log, level)."""
        r = self.ring
        ct = _as_u64(ct)
        nb = _lead(ct, (2, r.degree))
        if out is None:
            out = _empty(ct, tuple(ct.shape[:-2]) + (1 + int(level), r.degree))
        bi, bo = _Buf(ct), _Buf(out, True)
        if bo.count != nb * (1 + int(level)) * r.degree:
            raise FHEError(-9, "hoisted buffer must be [..., 1 + level, n]")
        w = _where(bi, bo)
        r._bind_stream(w)
        _check(lib().fhe_ct_hoist_batch(r._h, int(base_log), int(level), bi.ptr, bo.ptr, nb, w))
        return HoistedCiphertext(r, out, base_log, level, ct)

    def _hoisted_for(self, x, keys: "SwitchKey") -> "HoistedCiphertext":
        if keys.steps is None:
            raise FHEError(-9, "needs keys [nkeys, level, 2, n] (KeyGenerator.rotation_keys_for)")
        if not isinstance(x, HoistedCiphertext):
            return self.hoist(x, keys.base_log, keys.level)
        if (x.base_log, x.level) != (keys.base_log, keys.level):
            raise FHEError(-9, "the hoisted ciphertext and the keys differ in (base_log, level)")
        return x

    def _step_keys(self, steps, keys: "SwitchKey"):
        """(gs, key indices) of row-rotation steps in keys.g."""
        n = self.ring.degree
        have = {int(g): i for i, g in reversed(list(enumerate(keys.g)))}
        gs = [rotation_element(n, int(st)) for st in steps]
        missing = [int(st) for st, g in zip(steps, gs) if g not in have]
        if missing:
            raise FHEError(-9, "no key for rotation step(s) %s (KeyGenerator.rotation_keys_for)" % missing)
        return gs, [have[g] for g in gs]

    def rotate_many(self, ct, steps, keys: "SwitchKey", out=None):
        """Every row rotation in `steps` of ct (a ciphertext batch or a
        HoistedCiphertext) in one fhe_ct_hoisted_galois_batch call ->
        [..., len(steps), 2, n].  One key per step, looked up in keys.g."""
        r = self.ring
        h = self._hoisted_for(ct, keys)
        steps = [int(st) for st in steps]
        if not steps:
            raise FHEError(-9, "at least one step is needed")
        gs, idx = self._step_keys(steps, keys)
        nb = _lead(h.buf, (1 + h.level, r.degree))
        if out is None:
            out = _empty(h.buf, tuple(h.buf.shape[:-2]) + (len(steps), 2, r.degree))
        bh, bk, bo = _Buf(h.buf), _Buf(keys.key_ntt), _Buf(out, True)
        if bo.count != nb * len(steps) * 2 * r.degree:
            raise FHEError(-9, "output must be [..., len(steps), 2, n]")
        w = _where(bh, bk, bo)
        r._bind_stream(w)
        ns = len(steps)
        _check(lib().fhe_ct_hoisted_galois_batch(r._h, h.level, ns, (C.c_uint32 * ns)(*gs), (C.c_uint32 * ns)(*idx), bk.ptr,
                                                 bh.ptr, bo.ptr, nb, w))
        return out

    def prepare_plain(self, values, like=None) -> "PreparedPlaintext":
        """n slot values -> the plaintext linear_transform multiplies by,
        encoded with lift=True and transformed; resident where `like` is
        (a device tensor: on its device), else where `values` are."""
        return self._prepare_plains([values], like)[0]

    def _prepare_plains(self, values, like=None):
        """prepare_plain of a list of slot vectors in one encode and one transform."""
        n = self.ring.degree
        if all(_is_tensor(v) for v in values):
            v = torch.stack([x.reshape(n) for x in values])
        else:
            v = np.stack([np.asarray(H, dtype=np.uint64).reshape(n) for H in values])
            if _is_tensor(like):
                v = torch.from_numpy(v.view(np.int64)).to(like.device)
        coeff = self.simd.encode(v, True)
        rows = self.ring.forward_ntt(coeff)
        return [PreparedPlaintext(rows[i], coeff[i]) for i in range(len(values))]

    def linear_transform(self, ct, diagonals, keys: "SwitchKey", out=None):
        """sum over the items of `diagonals` {row-rotation step: plaintext} of
        plaintext (*) rotate(ct, step) -> [..., 2, n], in one
        fhe_ct_hoisted_linear_batch call: `level + 1` forward and two inverse
        transforms for the whole sum.  A plaintext is n slot values or a
        PreparedPlaintext (resident where the ciphertext is).  Step 0 (mod n/2)
        needs no key: it enters through multiply_plain and `accumulate`."""
        r = self.ring
        n = r.degree
        h = self._hoisted_for(ct, keys)
        rows, steps, zero = [], [], None
        items = list(diagonals.items())
        raw = [i for i, (_, pt) in enumerate(items) if not isinstance(pt, PreparedPlaintext)]
        if raw:
            for i, pt in zip(raw, self._prepare_plains([items[i][1] for i in raw], h.buf)):
                items[i] = (items[i][0], pt)
        for st, pt in items:
            if int(st) % (n // 2) == 0:
                zero = pt.coeff if zero is None else r.add(zero.reshape(1, n), pt.coeff.reshape(1, n))[0]
            else:
                rows.append(pt.row)
                steps.append(int(st))
        acc = 0
        if zero is not None:
            if h.ct is None:
                raise FHEError(-9, "step 0 needs the ciphertext itself (hoist() keeps it)")
            out = self.multiply_plain(h.ct, zero, out)
            acc = 1
        if not rows:
            if zero is None:
                raise FHEError(-9, "at least one diagonal is needed")
            return out
        gs, idx = self._step_keys(steps, keys)
        nb = _lead(h.buf, (1 + h.level, n))
        if out is None:
            out = _empty(h.buf, tuple(h.buf.shape[:-2]) + (2, n))
        pts = torch.stack(rows) if _is_tensor(rows[0]) else np.stack(rows)
        bh, bk, bp, bo = _Buf(h.buf), _Buf(keys.key_ntt), _Buf(pts), _Buf(out, True)
        if bo.count != nb * 2 * n:
            raise FHEError(-9, "output must be [..., 2, n]")
        w = _where(bh, bk, bp, bo)
        r._bind_stream(w)
        nt = len(steps)
        _check(lib().fhe_ct_hoisted_linear_batch(r._h, h.level, nt, (C.c_uint32 * nt)(*gs), (C.c_uint32 * nt)(*idx), bk.ptr,
                                                 bp.ptr, bh.ptr, acc, bo.ptr, nb, w))
        return out

    def matvec(self, ct, M, keys: "SwitchKey", out=None):
        """M v mod t for a D x D integer matrix M, D a power of two dividing
        n/2, and ct the encryption of v tiled with period D along both slot
        rows: diagonal j, diag_j[i] = M[i][(i + j) mod D] tiled, times the
        rotation by j, summed by linear_transform.  The result holds M v
        tiled.  `keys` holds the steps 1 .. D - 1 (rotation_keys_for)."""
        n = self.ring.degree
        M = np.asarray(M, dtype=object)
        D = int(M.shape[0]) if M.ndim == 2 else 0
        if D < 1 or M.shape[1] != D or (D & (D - 1)) or (n // 2) % D:
            raise FHEError(-9, "the matrix must be D x D with D a power of two dividing n/2")
        t = self.t or 4
        i = np.arange(D)
        diags = {}
        for j in range(D):
            d = np.array([int(M[a, (a + j) % D]) % t for a in i], dtype=np.uint64)
            diags[j] = np.tile(d, n // D)
        return self.linear_transform(ct, diags, keys, out)

    def inner_product_scaled(self, ct1, ct2, ek: EvaluationKey, keys: "SwitchKey", out=None):
        """<v, w> mod t in every slot of SIMD-encoded encryptions of v and w:
        multiply_scaled -> relinearize -> sum_slots."""
        return self.sum_slots(self.multiply_relin_scaled(ct1, ct2, ek), keys, False, out)


class BootstrapEngine:
    """The TFHE pieces of BootstrapEngine (bootstrap_engine.cpp) batched over
    ciphertexts: GLWE [..., k+1, n], GGSW [(k+1)*level, k+1, n], LWE masks
    [..., dim] with bodies [...]."""

    def __init__(self, ring: NTTProcessor, base_log: int, level: int, k: int = 1):
        self.ring, self.base_log, self.level, self.k = ring, base_log, level, k

    def prepare_ggsw(self, ggsw):
        """GGSW(s) [..., (k+1)*level, k+1, n] -> NTT-domain form (same shape)."""
        r, k, L = self.ring, self.k, self.level
        g = _as_u64(ggsw)
        nb = _lead(g, ((k + 1) * L, k + 1, r.degree))
        out = _like(g)
        bi, bo = _Buf(g), _Buf(out, True)
        w = _where(bi, bo)
        r._bind_stream(w)
        _check(lib().fhe_ggsw_prepare(r._h, k, L * nb, bi.ptr, bo.ptr, w))
        return out

    def external_product(self, glwe, ggsw_ntt, out=None):
        r = self.ring
        glwe = _as_u64(glwe)
        nb = _lead(glwe, (self.k + 1, r.degree))
        out = _like(glwe) if out is None else out
        bi, bk, bo = _Buf(glwe), _Buf(ggsw_ntt), _Buf(out, True)
        w = _where(bi, bk, bo)
        r._bind_stream(w)
        _check(lib().fhe_external_product_batch(r._h, self.k, self.base_log, self.level, bi.ptr, bk.ptr, bo.ptr,
                                                nb, w))
        return out

    def cmux(self, ggsw_ntt, ct0, ct1, out=None):
        """cmux (:520-540): ct0 + ggsw (x) (ct1 - ct0)."""
        r = self.ring
        ct0, ct1 = _as_u64(ct0), _as_u64(ct1)
        nb = _lead(ct0, (self.k + 1, r.degree))
        if tuple(ct1.shape) != tuple(ct0.shape):
            raise FHEError(-9, "ciphertext shapes differ")
        out = _like(ct0) if out is None else out
        bg, b0, b1, bo = _Buf(ggsw_ntt), _Buf(ct0), _Buf(ct1), _Buf(out, True)
        w = _where(bg, b0, b1, bo)
        r._bind_stream(w)
        _check(lib().fhe_cmux_batch(r._h, self.k, self.base_log, self.level, bg.ptr, b0.ptr, b1.ptr, bo.ptr, nb, w))
        return out

    def multiply_glwe_by_monomial(self, glwe, rotation, out=None):
        """multiply_glwe_by_monomial (:249-261); rotation: one int per ciphertext."""
        r = self.ring
        glwe = _as_u64(glwe)
        nb = _lead(glwe, (self.k + 1, r.degree))
        if _is_tensor(glwe):
            rot = torch.as_tensor(rotation, dtype=torch.int32, device=glwe.device).reshape(-1).contiguous()
            rp = rot.data_ptr()
        else:
            rot = np.ascontiguousarray(np.asarray(rotation, dtype=np.int32).reshape(-1))
            rp = rot.ctypes.data
        cnt = rot.numel() if _is_tensor(rot) else rot.size
        if cnt != nb:
            raise FHEError(-9, "one rotation per ciphertext")
        out = _like(glwe) if out is None else out
        bi, bo = _Buf(glwe), _Buf(out, True)
        w = _where(bi, bo)
        r._bind_stream(w)
        _check(lib().fhe_glwe_rotate_batch(r._h, self.k, rp, bi.ptr, bo.ptr, nb, w))
        return out

    def blind_rotate(self, acc, lwe_a, lwe_b, bsk_ntt, lwe_q: Optional[int] = None):
        """blind_rotate (:547-577), in place on acc [..., k+1, n]; lwe_a
        [..., dim], lwe_b [...]; bsk_ntt [dim, (k+1)*level, k+1, n] from
        prepare_ggsw.  lwe_q defaults to the ring modulus (:39-40)."""
        r = self.ring
        acc, lwe_a, lwe_b = _as_u64(acc), _as_u64(lwe_a), _as_u64(lwe_b)
        nb = _lead(acc, (self.k + 1, r.degree))
        dim = int(lwe_a.shape[-1])
        ba, bla, blb, bk = _Buf(acc, True), _Buf(lwe_a), _Buf(lwe_b), _Buf(bsk_ntt)
        if bla.count != nb * dim or blb.count != nb:
            raise FHEError(-9, "LWE masks must be [batch, dim] and bodies [batch]")
        w = _where(ba, bla, blb, bk)
        r._bind_stream(w)
        _check(lib().fhe_blind_rotate_batch(r._h, self.k, self.base_log, self.level, dim, bla.ptr, blb.ptr,
                                            lwe_q if lwe_q is not None else r.modulus, bk.ptr, ba.ptr, nb, w))
        return acc

    def repair_count(self) -> int:
        """Ciphertexts of this ring's two-CU blind rotations recomputed on one
        CU because a partner workgroup was not co-resident in time
        (fhe_br_repair_count; waits for the ring's stream)."""
        v = C.c_uint64(0)
        _check(lib().fhe_br_repair_count(self.ring._h, C.byref(v)))
        return int(v.value)

    def bootstrap(self, lwe_a, lwe_b, bsk_ntt, test_poly, ksk_a, ksk_b, ks_base_log: int, ks_level: int,
                  lwe_q: Optional[int] = None):
        """bootstrap_with_test_poly (bootstrap_engine.cpp:684-708) for a batch
        of LWE ciphertexts (lwe_a [..., dim], lwe_b [...]): blind rotation of
        (0, test_poly), sample extract, key switch (ksk_a [k*n*ks_level,
        out_dim], ksk_b [k*n*ks_level]).  -> (a [..., out_dim], b [...])."""
        r = self.ring
        lwe_a, lwe_b, test_poly, ksk_a, ksk_b = (_as_u64(x) for x in (lwe_a, lwe_b, test_poly, ksk_a, ksk_b))
        dim = int(lwe_a.shape[-1])
        nb = _lead(lwe_a, (dim,))
        out_dim = int(ksk_a.shape[-1])
        out_a = _empty(lwe_a, tuple(lwe_a.shape[:-1]) + (out_dim,))
        out_b = _like(lwe_b)
        bla, blb, bk, bt, bka, bkb, boa, bob = (_Buf(lwe_a), _Buf(lwe_b), _Buf(bsk_ntt), _Buf(test_poly), _Buf(ksk_a),
                                                _Buf(ksk_b), _Buf(out_a, True), _Buf(out_b, True))
        if blb.count != nb or bt.count != r.degree or bkb.count != self.k * r.degree * ks_level or \
                bka.count != bkb.count * out_dim:
            raise FHEError(-9, "LWE / test polynomial / key-switching key shapes disagree")
        w = _where(bla, blb, bk, bt, bka, bkb, boa, bob)
        r._bind_stream(w)
        _check(lib().fhe_bootstrap_batch(r._h, self.k, self.base_log, self.level, dim, bla.ptr, blb.ptr,
                                         lwe_q if lwe_q is not None else r.modulus, bk.ptr, bt.ptr, ks_base_log,
                                         ks_level, out_dim, bka.ptr, bkb.ptr, boa.ptr, bob.ptr, nb, w))
        return out_a, out_b

    programmable_bootstrap = bootstrap  # :716-722: the lookup table's polynomial as test_poly

    def create_lookup_table(self, func, input_modulus: int, output_modulus: int):
        """create_lookup_table (bootstrap_engine.cpp:725-758): the test
        polynomial encoding func (host-side, O(n))."""
        n, q = self.ring.degree, self.ring.modulus
        delta_out = q // output_modulus
        coeffs = np.zeros(n, dtype=np.uint64)
        for i in range(n):
            v = ((i * input_modulus + n) // (2 * n)) % input_modulus
            coeffs[i] = ((int(func(v)) % output_modulus) * delta_out) % q
        return coeffs

    def sample_extract(self, glwe):
        """sample_extract (:594-624) -> (a [..., k*n], b [...])."""
        r = self.ring
        glwe = _as_u64(glwe)
        nb = _lead(glwe, (self.k + 1, r.degree))
        lead = tuple(glwe.shape[:-2])
        a = _empty(glwe, lead + (self.k * r.degree,))
        b = _empty(glwe, lead if lead else (1,))
        bi, ba, bb = _Buf(glwe), _Buf(a, True), _Buf(b, True)
        w = _where(bi, ba, bb)
        r._bind_stream(w)
        _check(lib().fhe_sample_extract_batch(r._h, self.k, bi.ptr, ba.ptr, bb.ptr, nb, w))
        return a, b

    @staticmethod
    def key_switch(q: int, base_log: int, level: int, ksk_a, ksk_b, lwe_a, lwe_b, device: int = 0):
        """key_switch (:626-674): ksk_a [in_dim*level, out_dim], ksk_b
        [in_dim*level]; lwe_a [..., in_dim], lwe_b [...] -> (a, b)."""
        ksk_a, ksk_b, lwe_a, lwe_b = (_as_u64(x) for x in (ksk_a, ksk_b, lwe_a, lwe_b))
        in_dim = int(lwe_a.shape[-1])
        out_dim = int(ksk_a.shape[-1])
        nb = _lead(lwe_a, (in_dim,))
        out_a = _empty(lwe_a, tuple(lwe_a.shape[:-1]) + (out_dim,))
        out_b = _like(lwe_b)
        bka, bkb, bla, blb, boa, bob = (_Buf(ksk_a), _Buf(ksk_b), _Buf(lwe_a), _Buf(lwe_b), _Buf(out_a, True),
                                        _Buf(out_b, True))
        if bka.count != in_dim * level * out_dim or bkb.count != in_dim * level or blb.count != nb:
            raise FHEError(-9, "key switching key / LWE shapes disagree")
        w = _where(bka, bkb, bla, blb, boa, bob)
        s = _stream_ptr() if w == FHE_DEVICE else None
        _check(lib().fhe_key_switch_batch(q, base_log, level, in_dim, out_dim, bka.ptr, bkb.ptr, bla.ptr, blb.ptr,
                                          boa.ptr, bob.ptr, nb, w, device, s))
        return out_a, out_b

    def slot_extract(self, cts, slots, offsets=None, ref=None, negate: bool = False, out=None):
        """The LWE ciphertexts at coefficients `slots` of cts - ref (negate:
        ref - cts; ref None, one ciphertext [2, n] or the shape of cts), the
        RLWE (c0, c1) read as the GLWE (mask c1, body c0), bodies plus
        offsets[s] mod q (fhe_slot_extract_batch): cts [..., 2, n] ->
        (a [..., S, n], b [..., S]).  The words of subtract (or negate),
        multiply_glwe_by_monomial by -slot, sample_extract and a modular add
        on the body, in one launch.  out: an (a, b) pair to write into."""
        r = self.ring
        if self.k != 1:
            raise FHEError(-9, "slot_extract takes RLWE ciphertexts (k = 1)")
        cts = _as_u64(cts)
        nb = _lead(cts, (2, r.degree))
        slots = [int(s) for s in slots]
        S = len(slots)
        if any(s < 0 or s >= 1 << 32 for s in slots):
            raise FHEError(-9, "slot index out of range")
        if offsets is not None:
            offsets = [int(o) & ((1 << 64) - 1) for o in offsets]
            if len(offsets) != S:
                raise FHEError(-9, "one offset per slot")
        be, cnt = None, 0
        if ref is not None:
            ref = _as_u64(ref)
            if tuple(ref.shape) == (2, r.degree):
                be, cnt = _Buf(ref), 1
            elif tuple(ref.shape) == tuple(cts.shape):
                be, cnt = _Buf(ref), nb
            else:
                raise FHEError(-9, "ciphertext shapes differ")
        lead = tuple(cts.shape[:-2])
        a, b = out if out is not None else (_empty(cts, lead + (S, r.degree)), _empty(cts, lead + (S,)))
        bc, ba, bb = _Buf(cts), _Buf(a, True), _Buf(b, True)
        if ba.count != nb * S * r.degree or bb.count != nb * S:
            raise FHEError(-9, "outputs must be [..., S, n] and [..., S]")
        w = _where(bc, be, ba, bb)
        r._bind_stream(w)
        _check(lib().fhe_slot_extract_batch(r._h, bc.ptr, be.ptr if be else None, cnt, int(bool(negate)),
                                            (C.c_uint32 * max(1, S))(*slots),
                                            (C.c_uint64 * max(1, S))(*offsets) if offsets is not None else None, S,
                                            ba.ptr, bb.ptr, nb, w))
        return a, b

    @staticmethod
    def lwe_sum(q: int, lwe_a, lwe_b, body_offset: int = 0, device: int = 0, out=None):
        """Sum over the leading axis of LWE ciphertexts (fhe_lwe_sum_batch):
        lwe_a [terms, ..., dim], lwe_b [terms, ...] -> (a [..., dim], b [...]),
        b = sum + body_offset, all mod q."""
        lwe_a, lwe_b = _as_u64(lwe_a), _as_u64(lwe_b)
        if len(lwe_a.shape) < 2 or tuple(lwe_a.shape[:-1]) != tuple(lwe_b.shape):
            raise FHEError(-9, "LWE masks must be [terms, ..., dim] and bodies [terms, ...]")
        terms, dim = int(lwe_a.shape[0]), int(lwe_a.shape[-1])
        a, b = out if out is not None else (_empty(lwe_a, tuple(lwe_a.shape[1:])), _empty(lwe_b, tuple(lwe_b.shape[1:])))
        bla, blb, boa, bob = _Buf(lwe_a), _Buf(lwe_b), _Buf(a, True), _Buf(b, True)
        nb = blb.count // terms if terms else 0
        if boa.count != nb * dim or bob.count != nb:
            raise FHEError(-9, "outputs must be [..., dim] and [...]")
        w = _where(bla, blb, boa, bob)
        s = _stream_ptr() if w == FHE_DEVICE else None
        _check(lib().fhe_lwe_sum_batch(q, dim, bla.ptr, blb.ptr, terms, int(body_offset) & ((1 << 64) - 1), boa.ptr,
                                       bob.ptr, nb, w, device, s))
        return a, b


class Comparisons:
    """Encrypted comparisons of packed slot values (the fraud-detection surface
    of encryption.cpp:1112-1303, which stops at "the difference, ready for
    PBS"): each operation returns, per ciphertext and slot, an LWE ciphertext
    (a [..., S, dim], b [..., S]) under the bootstrapping key's LWE key whose
    phase is about delta = q / t when the predicate holds and about 0
    otherwise (detect_duplicate: delta times the number of matches).

    SIGN(D, off) = slot_extract with body offsets off, key_switch from n to the
    LWE dimension, bootstrap with the CONSTANT test polynomial h = delta / 2:
    phase +h for an input phase in [0, q / 2), -h otherwise.  Slot values lie
    in [0, t / 2); h centres each value in its window.  Both SIGN halves of an
    operation go through one key switch and one bootstrap, stacked along the
    batch, and lwe_sum adds them.  bsk_ntt is prepare_ggsw's form; ksk_a
    [n * ks_level, dim] and ksk_b serve both key switches, as in bootstrap."""

    def __init__(self, ring: NTTProcessor, t: int, bsk_ntt, ksk_a, ksk_b, base_log: int, level: int,
                 ks_base_log: int, ks_level: int):
        self.ring, self.t = ring, (t if t else 4)
        self.bsk_ntt, self.ksk_a, self.ksk_b = bsk_ntt, _as_u64(ksk_a), _as_u64(ksk_b)
        self.ks_base_log, self.ks_level = ks_base_log, ks_level
        self.engine = BootstrapEngine(ring, base_log, level, 1)
        self.dim = int(self.ksk_a.shape[-1])
        q = ring.modulus
        self.delta = q // self.t
        self.half = self.delta // 2
        tp = np.full(ring.degree, self.half, dtype=np.uint64)
        self.sign_poly = torch.from_numpy(tp.view(np.int64)).to(self.ksk_a.device) if _is_tensor(self.ksk_a) else tp

    def encode(self, v: int) -> int:
        """encode_plaintext's word (encryption.cpp:107-115): (v delta mod 2^64) % q."""
        return ((int(v) * self.delta) & ((1 << 64) - 1)) % self.ring.modulus

    def _sum_signs(self, halves, slots, body_offset):
        """halves: (cts, ref, negate, offsets) per SIGN term."""
        r, q, S = self.ring, self.ring.modulus, len(slots)
        cts0 = _as_u64(halves[0][0])
        lead = tuple(cts0.shape[:-2])
        H = len(halves)
        ea = _empty(cts0, (H,) + lead + (S, r.degree))
        eb = _empty(cts0, (H,) + lead + (S,))
        for i, (cts, ref, negate, offs) in enumerate(halves):
            self.engine.slot_extract(cts, slots, [o % q for o in offs], ref, negate, out=(ea[i], eb[i]))
        dev = cts0.device.index or 0 if _is_tensor(cts0) else r.device
        la, lb = BootstrapEngine.key_switch(q, self.ks_base_log, self.ks_level, self.ksk_a, self.ksk_b, ea, eb, dev)
        sa, sb = self.engine.bootstrap(la, lb, self.bsk_ntt, self.sign_poly, self.ksk_a, self.ksk_b, self.ks_base_log,
                                       self.ks_level)
        return BootstrapEngine.lwe_sum(q, sa, sb, body_offset, dev)

    def greater_equal(self, a, b, slots):
        """[a >= b] per slot: SIGN(a - b, h) + h."""
        return self._sum_signs([(a, b, False, [self.half] * len(slots))], slots, self.half)

    def greater_than(self, a, b, slots, _negate=False):
        """[a > b] (compare_greater_than :1174): SIGN(a - b, h - delta) + h."""
        return self._sum_signs([(a, b, _negate, [self.half - self.delta] * len(slots))], slots, self.half)

    def less_than(self, a, b, slots):
        """[a < b] (compare_less_than :1197-1204): greater_than(b, a), the
        difference negated in the extraction."""
        return self.greater_than(a, b, slots, _negate=True)

    def check_threshold(self, tally, thresholds, slots):
        """[tally >= thresholds[s]] per slot (check_threshold :1112-1143):
        SIGN(tally, h - encode(thr[s])) + h."""
        if len(thresholds) != len(slots):
            raise FHEError(-9, "one threshold per slot")
        return self._sum_signs([(tally, None, False, [self.half - self.encode(v) for v in thresholds])], slots,
                               self.half)

    def equal(self, a, b, slots):
        """[a == b] (compare_equal :1206): SIGN(a - b, h) + SIGN(b - a, h)."""
        offs = [self.half] * len(slots)
        return self._sum_signs([(a, b, False, offs), (a, b, True, offs)], slots, 0)

    def check_range(self, ct, lo: int, hi: int, slots):
        """[lo <= ct <= hi] (check_range :1228): SIGN(ct, h - encode(lo)) +
        SIGN(-ct, h + encode(hi)).  lo <= hi: with an empty range both terms
        would be -h and the sum would leave the {0, delta} encoding."""
        if lo > hi:
            raise FHEError(-9, "check_range needs min <= max")
        S = len(slots)
        return self._sum_signs([(ct, None, False, [self.half - self.encode(lo)] * S),
                                (ct, None, True, [self.half + self.encode(hi)] * S)], slots, 0)

    def detect_duplicate(self, new, existing, slots):
        """The number of `existing` ciphertexts equal to `new` per slot
        (detect_duplicate :1293-1300, "add the equality tests"): the 2 count
        SIGN terms of equal(new, existing_i) in one sum.  An empty list gives
        the all-zero LWE."""
        offs = [self.half] * len(slots)
        if len(existing) == 0:
            new = _as_u64(new)
            lead = tuple(new.shape[:-2]) + (len(slots),)
            if _is_tensor(new):
                return (torch.zeros(lead + (self.dim,), dtype=new.dtype, device=new.device),
                        torch.zeros(lead, dtype=new.dtype, device=new.device))
            return np.zeros(lead + (self.dim,), dtype=np.uint64), np.zeros(lead, dtype=np.uint64)
        halves = [(new, e, neg, offs) for e in existing for neg in (False, True)]
        return self._sum_signs(halves, slots, 0)

    @staticmethod
    def pack(result, slots, pack_key: "PackKey", engine: "EncryptionEngine", out=None, accumulate: bool = False):
        """A comparison result (a, b) back as one BFV ciphertext per leading
        index, bit s at coefficient slots[s] (EncryptionEngine.pack_lwe)."""
        return engine.pack_lwe(result[0], result[1], slots, pack_key, out, accumulate)


def decompose_polynomial(ring: NTTProcessor, poly, base_log: int, level: int, out=None):
    """BootstrapEngine::decompose_polynomial (bootstrap_engine.cpp:152-185);
    poly [..., n] -> [..., level, n]."""
    poly = _as_u64(poly)
    nb = ring._batch(poly)
    if out is None:
        shape = tuple(poly.shape[:-1]) + (level, ring.degree)
        out = torch.empty(shape, dtype=poly.dtype, device=poly.device) if _is_tensor(poly) else np.empty(
            shape, dtype=np.uint64)
    bi, bo = _Buf(poly), _Buf(out, True)
    w = _where(bi, bo)
    ring._bind_stream(w)
    _check(lib().fhe_decompose_batch(ring._h, base_log, level, bi.ptr, bo.ptr, nb, w))
    return out


# ----------------------------------------------------------------- modular arithmetic
def modmul_batch(q: int, a, b, out=None, device: int = 0):
    """BarrettReducer::barrett_mul contract, batched on the GPU: a*b mod q."""
    a, b = _as_u64(a), _as_u64(b)
    out = _like(a) if out is None else out
    ba, bb, bo = _Buf(a), _Buf(b), _Buf(out, True)
    if not (ba.count == bb.count == bo.count):
        raise FHEError(-9, "operand sizes differ")
    w = _where(ba, bb, bo)
    s = _stream_ptr() if w == FHE_DEVICE else None
    _check(lib().fhe_modmul_batch(q, ba.ptr, bb.ptr, bo.ptr, ba.count, w, device, s))
    return out


class BarrettReducer:
    """BarrettReducer(modulus) (modular_arithmetic.cpp:238-280)."""

    def __init__(self, modulus: int):
        if modulus == 0:
            raise FHEError(-8, "Modulus must be non-zero for Barrett reduction")
        self.modulus = modulus

    def barrett_mul_batch(self, a, b, out=None, device: int = 0):
        return modmul_batch(self.modulus, a, b, out, device)

    def barrett_mul(self, a: int, b: int) -> int:
        return int(self.barrett_mul_batch(np.array([a], np.uint64), np.array([b], np.uint64))[0])


class MultiLimbModularArithmetic:
    """2-limb MultiLimbModularArithmetic (modular_arithmetic.cpp:471-693)."""

    def __init__(self, modulus_limbs):
        self.q = (C.c_uint64 * 2)(*[int(x) for x in modulus_limbs])
        k = (C.c_uint64 * 7)()
        _check(lib().fhe_ml_constants(self.q, k))
        self.constants = list(k)

    def montgomery_mul_batch(self, a, b, out=None, device: int = 0):
        """a, b: [..., 2] little-endian limbs."""
        a, b = _as_u64(a), _as_u64(b)
        out = _like(a) if out is None else out
        ba, bb, bo = _Buf(a), _Buf(b), _Buf(out, True)
        if ba.count % 2 or not (ba.count == bb.count == bo.count):
            raise FHEError(-9, "operands must be [..., 2] limb arrays of equal size")
        w = _where(ba, bb, bo)
        s = _stream_ptr() if w == FHE_DEVICE else None
        _check(lib().fhe_ml_montmul_batch(self.q, ba.ptr, bb.ptr, bo.ptr, ba.count // 2, w, device, s))
        return out


class ModularArithmetic:
    """The N-API ``ModularArithmetic`` class (index.d.ts:32-44,
    src/native/lib.rs:42-121) with the reference's exact constants."""

    def __init__(self, modulus: int):
        if modulus <= 0:
            raise FHEError(-9, "Modulus must be positive")
        self._k = (C.c_uint64 * 4)()
        _check(lib().fhe_mont_constants_compat(modulus, self._k))
        self.modulus = modulus

    @staticmethod
    def _nn(*xs):
        for x in xs:
            if x < 0:
                raise FHEError(-9, "Inputs must be non-negative")

    def montgomery_mul(self, a, b):
        self._nn(a, b)
        return lib().fhe_compat_montgomery_mul(self._k, a, b)

    def mod_add(self, a, b):
        self._nn(a, b)
        return lib().fhe_compat_mod_add(self.modulus, a, b)

    def mod_sub(self, a, b):
        self._nn(a, b)
        return lib().fhe_compat_mod_sub(self.modulus, a, b)

    def to_montgomery(self, a):
        self._nn(a)
        return lib().fhe_compat_to_montgomery(self._k, a)

    def from_montgomery(self, a):
        self._nn(a)
        return lib().fhe_compat_from_montgomery(self._k, a)

    def get_modulus(self):
        return self.modulus

    @property
    def constants(self):
        return list(self._k)


# ----------------------------------------------------------------- timing helper
class HipEvent:
    """hipEvent on an explicit stream (for kernel timing in bench.py)."""

    def __init__(self):
        h = C.c_void_p()
        _check(lib().fhe_event_create(C.byref(h)))
        self._h = h

    def record(self, stream_ptr):
        _check(lib().fhe_event_record(self._h, C.c_void_p(stream_ptr)))

    def elapsed_ms(self, end: "HipEvent") -> float:
        ms = C.c_float()
        _check(lib().fhe_event_elapsed_ms(self._h, end._h, C.byref(ms)))
        return ms.value

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and _lib is not None:
            _lib.fhe_event_destroy(h)
