"""lol_amd/tensor.py — ctypes binding of include/lolhip.h, shaped like Lol's `Tensor` class.

Method names follow the reference's class methods (lol/Crypto/Lol/Cyclotomic/Tensor.hs:86-193):
crt, crtInv, l, lInv, mulGPow, mulGDec, divGPow, divGDec, mulGCRT, divGCRT,
twacePowDec, twaceCRT, embedPow, embedDec, embedCRT, plus zipWithT (*) as `mul` and
the fused ring product `polymul` (Cyc (*), lol/Crypto/Lol/Cyclotomic/Cyc.hs:262-297).

Arrays are int64 with shape [..., n, T] (T = number of RNS moduli; a trailing axis of
length 1 for a single modulus) — the reference's AoS layout (tensor.h:69).
`divG*` return None where the reference returns Nothing (CPP.hs:309-323).
The same six L / G methods over the class's other element types (int64, float64, complex128 slabs) are `eltOp` and its
wrappers `lR`, `lInvR`, `mulGPowR`, `mulGDecR`, `divGPowR`, `divGDecR`; `mulC` is the complex pointwise product.

Two calling styles per operation:
  * numpy arrays  -> host round trip through `lolhip_op_host`
  * torch CUDA int64 tensors (or raw device pointers via *_dev) -> in place in HBM
Neither has a CPU fallback.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_i64p = C.POINTER(C.c_int64)
_i32p = C.POINTER(C.c_int32)

OK, ERR_INVALID, ERR_MODULUS, ERR_NO_CRT, ERR_ROOT, ERR_NO_DEVICE, ERR_HIP, ERR_NOT_DIVISIBLE, ERR_DEVICE = 0, -1, -2, -3, -4, -5, -6, -7, -8
_ERRNAMES = {ERR_INVALID: "invalid argument", ERR_MODULUS: "modulus out of range / missing inverse",
             ERR_NO_CRT: "no CRT basis for this modulus", ERR_ROOT: "bad root of unity",
             ERR_NO_DEVICE: "no HIP device (liblolhip has no CPU fallback)", ERR_HIP: "HIP runtime error",
             ERR_NOT_DIVISIBLE: "not divisible by g",
             ERR_DEVICE: "the current HIP device is not the plan's device"}

OP_CRT, OP_CRTINV, OP_MUL, OP_POLYMUL, OP_L, OP_LINV, OP_MULGPOW, OP_MULGDEC, OP_DIVGPOW, OP_DIVGDEC, OP_MULGCRT, OP_DIVGCRT = range(12)
EXT_TWACE_POWDEC, EXT_TWACE_CRT, EXT_EMBED_POW, EXT_EMBED_DEC, EXT_EMBED_CRT, EXT_COEFFS = range(6)
ELT_I64, ELT_F64, ELT_C64 = range(3)


class LolHipError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        super().__init__(f"lolhip: {_ERRNAMES.get(code, code)} ({code}) {what}")


class NoDeviceError(LolHipError):
    pass


class _PP(C.Structure):
    _fields_ = [("prime", C.c_int16), ("exponent", C.c_int16)]


def lib_path() -> str:
    return os.path.join(_HERE, "liblolhip.so")


_lib = None


def lib():
    """Load liblolhip.so (built in-tree by __graft_entry__.build()).  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm wheels carry their own libamdhip64; if torch is going to be used in this
    # process it must be the one that loads the HIP runtime first, or its later device probe
    # finds the GPU already claimed by a second runtime copy ("No HIP GPUs are available").
    if os.environ.get("LOLHIP_NO_TORCH_PRELOAD") is None:
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)")
    L = C.CDLL(path)
    vp, i64, ci = C.c_void_p, C.c_int64, C.c_int
    pp = C.POINTER(_PP)
    L.lolhip_plan_create.argtypes = [pp, ci, _i64p, ci, ci, C.POINTER(vp)]
    L.lolhip_plan_create_roots.argtypes = [pp, ci, _i64p, ci, _i64p, _i64p, ci, C.POINTER(vp)]
    L.lolhip_plan_destroy.argtypes = [vp]
    L.lolhip_plan_destroy.restype = None
    for nm in ("lolhip_plan_n", "lolhip_plan_m"):
        getattr(L, nm).argtypes = [vp]
        getattr(L, nm).restype = i64
    L.lolhip_plan_T.argtypes = [vp]
    L.lolhip_plan_has_crt.argtypes = [vp]
    L.lolhip_plan_table.argtypes = [vp, ci, ci, _i64p, i64]
    L.lolhip_plan_table.restype = i64
    L.lolhip_good_q.argtypes = [i64, i64]
    L.lolhip_good_q.restype = i64
    for nm in ("crt", "crtinv", "l", "linv", "mulgpow", "mulgdec", "divgpow", "divgdec", "mulgcrt", "divgcrt"):
        getattr(L, f"lolhip_{nm}_batch").argtypes = [vp, vp, vp, i64]
    L.lolhip_mul_batch.argtypes = [vp, vp, vp, vp, i64]
    for nm in ("crtc", "crtinvc", "gaussian_dec"):
        getattr(L, f"lolhip_{nm}_batch").argtypes = [vp, vp, vp, i64]
    L.lolhip_polymul_batch.argtypes = [vp, vp, vp, vp, vp, i64]
    L.lolhip_ctmul_crt_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i64]
    L.lolhip_decompose_len.argtypes = [vp, i64]
    L.lolhip_gadget.argtypes = [vp, i64, _i64p, i64]
    L.lolhip_decompose_batch.argtypes = [vp, vp, vp, i64, vp, i64]
    L.lolhip_knapsack_batch.argtypes = [vp, vp, vp, ci, vp, ci, vp, vp, i64]
    L.lolhip_keyswitch_batch.argtypes = [vp, vp, vp, i64, vp, ci, vp, vp, vp, i64]
    L.lolhip_rescale_drop_batch.argtypes = [vp, vp, vp, vp, i64]
    L.lolhip_decrypt_work_len.argtypes = [vp, ci, i64]
    L.lolhip_decrypt_work_len.restype = i64
    L.lolhip_error_term_batch.argtypes = [vp, vp, vp, ci, ci, vp, ci, i64, vp, vp, i64]
    L.lolhip_decrypt_batch.argtypes = [vp, vp, vp, vp, vp, ci, ci, vp, ci, i64, i64, vp, vp, i64]
    L.lolhip_encrypt_work_len.argtypes = [vp, i64]
    L.lolhip_encrypt_work_len.restype = i64
    L.lolhip_encrypt_batch.argtypes = [vp, vp, vp, vp, vp, vp, C.c_double, C.c_char_p, C.c_uint64, ci, vp, vp, i64]
    L.lolhip_error_rounded_batch.argtypes = [vp, vp, C.c_double, C.c_char_p, C.c_uint64, vp, vp, i64]
    L.lolhip_kshint_work_len.argtypes = [vp, i64, i64]
    L.lolhip_kshint_work_len.restype = i64
    L.lolhip_kshint_batch.argtypes = [vp, vp, vp, vp, C.c_double, i64, C.c_char_p, C.c_uint64, vp, vp, i64]
    L.lolhip_tunnel_hint_work_len.argtypes = [vp, vp, i64]
    L.lolhip_tunnel_hint_work_len.restype = i64
    L.lolhip_tunnel_hint_batch.argtypes = [vp, vp, vp, vp, vp, vp, C.c_double, i64, C.c_char_p, C.c_uint64, vp, vp]
    L.lolhip_khprf_create.argtypes = [vp, i64, _i32p, ci, _i64p, _i64p, C.POINTER(vp)]
    L.lolhip_khprf_create_lifted.argtypes = [vp, vp, i64, _i32p, ci, _i64p, _i64p, C.POINTER(vp)]
    L.lolhip_khprf_destroy.argtypes = [vp]
    L.lolhip_khprf_destroy.restype = None
    L.lolhip_khprf_work_len.argtypes = [vp, i64, i64]
    L.lolhip_khprf_work_len.restype = i64
    L.lolhip_khprf_eval_batch.argtypes = [vp, vp, i64, i64, vp, vp]
    L.lolhip_khprf_batch.argtypes = [vp, vp, vp, ci, i64, i64, i64, vp, vp]
    L.lolhip_encode_scales.argtypes = [vp, i64, ci, _i64p, _i64p]
    L.lolhip_ct_lincomb_batch.argtypes = [vp, vp, vp, ci, _i64p, vp, ci, _i64p, vp, i64]
    L.lolhip_public_work_len.argtypes = [vp, vp, i64]
    L.lolhip_public_work_len.restype = i64
    L.lolhip_add_public_batch.argtypes = [vp, vp, vp, vp, vp, i64, vp, ci, ci, ci, ci, i64, i64, i64, vp, _i64p, vp, i64]
    L.lolhip_mul_public_batch.argtypes = [vp, vp, vp, vp, i64, i64, vp, ci, ci, vp, vp, i64]
    L.lolhip_modswitch_work_len.argtypes = [vp, vp, ci, i64]
    L.lolhip_modswitch_work_len.restype = i64
    L.lolhip_modswitch_batch.argtypes = [vp, vp, vp, vp, ci, ci, ci, i64, i64, vp, ci, _i64p, vp, i64]
    L.lolhip_tunnel_chain_create.argtypes = [ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i64, vp, vp,
                                             C.POINTER(vp)]
    L.lolhip_tunnel_chain_destroy.argtypes = [vp]
    L.lolhip_tunnel_chain_destroy.restype = None
    L.lolhip_tunnel_chain_work_len.argtypes = [vp, i64]
    L.lolhip_tunnel_chain_work_len.restype = i64
    L.lolhip_tunnel_chain_batch.argtypes = [vp, vp, vp, ci, ci, i64, i64, vp, ci, _i64p, vp, i64]
    L.lolhip_ct_affine_mul_batch.argtypes = [vp, vp, vp, _i64p, vp, vp, _i64p, vp, ci, vp, i64]
    L.lolhip_ptround_create.argtypes = [ci, i64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i64, vp, vp, vp, C.POINTER(vp)]
    L.lolhip_ptround_destroy.argtypes = [vp]
    L.lolhip_ptround_destroy.restype = None
    L.lolhip_ptround_work_len.argtypes = [vp, i64]
    L.lolhip_ptround_work_len.restype = i64
    L.lolhip_ptround_batch.argtypes = [vp, vp, vp, ci, ci, i64, i64, vp, ci, _i64p, _i64p, vp, i64]
    L.lolhip_crtset_dec.argtypes = [pp, ci, pp, ci, i64, _i64p, i64]
    L.lolhip_crtset_modulus.argtypes = [pp, ci, i64, ci]
    L.lolhip_crtset_host.argtypes = [pp, ci, pp, ci, i64, ci, _i64p, i64]
    L.lolhip_crtset.argtypes = [vp, pp, ci, pp, ci, i64, ci, vp, vp, i64]
    L.lolhip_pt_tunnel_modulus.argtypes = [pp, ci, pp, ci, i64, ci, i64, ci]
    for nm in ("crtset_dec", "crtset_modulus", "crtset_host", "crtset", "pt_tunnel_modulus"):
        getattr(L, f"lolhip_{nm}").restype = i64
    L.lolhip_pt_tunnel_create.argtypes = [ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(_i64p), i64, ci, C.POINTER(vp)]
    L.lolhip_pt_tunnel_destroy.argtypes = [vp]
    L.lolhip_pt_tunnel_destroy.restype = None
    L.lolhip_pt_tunnel_work_len.argtypes = [vp, i64]
    L.lolhip_pt_tunnel_work_len.restype = i64
    L.lolhip_pt_tunnel_batch.argtypes = [vp, vp, vp, vp, vp, i64]
    L.lolhip_ringmul_moduli.argtypes = [pp, ci, _i64p, ci, _i64p]
    L.lolhip_ringmul_create.argtypes = [vp, vp, C.POINTER(vp)]
    L.lolhip_ringmul_destroy.argtypes = [vp]
    L.lolhip_ringmul_destroy.restype = None
    L.lolhip_ringmul_work_len.argtypes = [vp, i64]
    L.lolhip_ringmul_work_len.restype = i64
    L.lolhip_ringmul_batch.argtypes = [vp, vp, vp, vp, vp, vp, i64]
    L.lolhip_ringmul_prepare.argtypes = [vp, vp, vp, vp, vp, i64]
    L.lolhip_ringmul_prepared_batch.argtypes = [vp, vp, vp, vp, vp, i64, vp, i64]
    L.lolhip_gadget_correct_work_len.argtypes = [vp, i64, ci, i64]
    L.lolhip_gadget_correct_work_len.restype = i64
    L.lolhip_gadget_correct_batch.argtypes = [vp, vp, vp, i64, ci, vp, vp, vp, i64]
    L.lolhip_gadget_encode_batch.argtypes = [vp, vp, vp, i64, vp, vp, i64]
    L.lolhip_gsqnorm_batch.argtypes = [vp, vp, vp, vp, i64]
    L.lolhip_gsqnorm_f64_batch.argtypes = [vp, vp, vp, vp, i64]
    L.lolhip_rlwe_work_len.argtypes = [vp, ci, i64]
    L.lolhip_rlwe_work_len.restype = i64
    L.lolhip_rlwe_secret.argtypes = [vp, vp, C.c_char_p, C.c_uint64, vp]
    L.lolhip_rlwe_sample_batch.argtypes = [vp, vp, ci, i64, vp, C.c_double, C.c_char_p, C.c_uint64, vp, vp, vp, i64]
    L.lolhip_rlwe_error_batch.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp, i64]
    L.lolhip_rlwr_rounded_prod_batch.argtypes = [vp, i64, vp, vp, vp, vp, vp, i64]
    L.lolhip_rlwr_check_batch.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, i64]
    L.lolhip_rlwe_error_bound.argtypes = [pp, ci, C.c_double, C.c_double, ci, C.POINTER(C.c_double)]
    L.lolhip_chacha20_block.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.lolhip_chacha20_block.restype = None
    L.lolhip_ext_create.argtypes = [vp, vp, C.POINTER(vp)]
    L.lolhip_ext_destroy.argtypes = [vp]
    L.lolhip_ext_destroy.restype = None
    for nm in ("twace_powdec", "twace_crt", "embed_pow", "embed_dec", "embed_crt", "coeffs"):
        getattr(L, f"lolhip_{nm}_batch").argtypes = [vp, vp, vp, vp, i64]
    L.lolhip_evallin_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64]
    L.lolhip_tunnel_work_len.argtypes = [vp, vp, i64, i64]
    L.lolhip_tunnel_work_len.restype = i64
    L.lolhip_tunnel_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, i64]
    L.lolhip_ext_table.argtypes = [vp, ci, _i32p, i64]
    L.lolhip_ext_table.restype = i64
    L.lolhip_op_host.argtypes = [vp, ci, _i64p, _i64p, i64]
    L.lolhip_ext_host.argtypes = [vp, ci, _i64p, _i64p, i64]
    L.lolhip_thread_release.argtypes = []
    L.lolhip_thread_release.restype = None
    u8p = C.POINTER(C.c_uint8)
    L.lolhip_rqproduct_read.argtypes = [u8p, i64, C.POINTER(C.c_uint32), _i64p, ci, C.POINTER(ci), _i64p, i64]
    L.lolhip_rqproduct_read.restype = i64
    L.lolhip_rqproduct_write.argtypes = [C.c_uint32, _i64p, ci, _i64p, i64, u8p, i64]
    L.lolhip_rqproduct_write.restype = i64
    L.lolhip_kshint_read.argtypes = [u8p, i64, C.POINTER(C.c_uint32), _i64p, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), _i64p, i64]
    L.lolhip_kshint_read.restype = i64
    u32p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    L.lolhip_r_read.argtypes = [u8p, i64, u32p, _i64p, i64]
    L.lolhip_secretkey_read.argtypes = [u8p, i64, u32p, f64p, _i64p, i64]
    L.lolhip_kqproduct_read.argtypes = [u8p, i64, u32p, _i64p, ci, C.POINTER(ci), f64p, i64]
    L.lolhip_linearrq_read.argtypes = [u8p, i64, u32p, u32p, C.POINTER(ci), u32p, _i64p, ci, C.POINTER(ci), _i64p, i64]
    L.lolhip_kshint_write.argtypes = [C.c_uint32, _i64p, ci, ci, ci, _i64p, i64, C.c_uint64, C.c_uint64, u8p, i64]
    L.lolhip_tunnelhint_read.argtypes = [u8p, i64, u32p, u32p, u32p, C.POINTER(C.c_uint64), _i64p, _i64p, _i64p, _i64p, ci]
    u8pp = C.POINTER(C.POINTER(C.c_uint8))
    L.lolhip_r_write.argtypes = [C.c_uint32, _i64p, i64, u8p, i64]
    L.lolhip_secretkey_write.argtypes = [C.c_uint32, C.c_double, _i64p, i64, u8p, i64]
    L.lolhip_linearrq_write.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, _i64p, ci, ci, _i64p, i64, u8p, i64]
    L.lolhip_tunnelhint_write.argtypes = [u8p, i64, u8pp, _i64p, ci, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, u8p, i64]
    L.lolhip_chain_read.argtypes = [u8p, i64, _i64p, _i64p, ci]
    L.lolhip_chain_write.argtypes = [u8pp, _i64p, ci, u8p, i64]
    for nm in ("r_write", "secretkey_write", "linearrq_write", "tunnelhint_write", "chain_read", "chain_write"):
        getattr(L, f"lolhip_{nm}").restype = i64
    for nm in ("r_read", "secretkey_read", "kqproduct_read", "linearrq_read", "kshint_write", "tunnelhint_read"):
        getattr(L, f"lolhip_{nm}").restype = i64
    L.lolhip_elt_op_batch.argtypes = [vp, vp, ci, ci, ci, vp, vp, i64]
    L.lolhip_mulc_batch.argtypes = [vp, vp, vp, i64]
    L.lolhip_debug_set.argtypes = [C.c_char_p, ci]
    L.lolhip_copy_slab.argtypes = [vp, vp, vp, i64, ci]
    L.lolhip_device_count.restype = ci
    L.lolhip_version.restype = C.c_char_p
    L.lolhip_last_status.restype = ci
    _lib = L
    return L


def _check(rc, what=""):
    if rc == OK:
        return
    raise (NoDeviceError if rc == ERR_NO_DEVICE else LolHipError)(rc, what)


def device_count() -> int:
    return lib().lolhip_device_count()


def debug_set(name: str, value: bool) -> None:
    """Force (value true) or release a launch path of the library: lolhip_debug_set (tests, A/B runs)."""
    _check(lib().lolhip_debug_set(name.encode(), 1 if value else 0), f"lolhip_debug_set({name})")


def good_q(m: int, lower: int) -> int:
    """Head of `goodQs m lower` (ZqBasic.hs:71-73)."""
    return int(lib().lolhip_good_q(m, lower))


def factor_pps(m: int):
    """ppsFact (FactoredDefs.hs:360-361): [(p, e)] ascending."""
    out, p = [], 2
    while m > 1:
        if m % p == 0:
            e = 0
            while m % p == 0:
                m //= p
                e += 1
            out.append((p, e))
        p += 1 if p == 2 else 2
        if p * p > m and m > 1:
            out.append((m, 1))
            break
    return out


def _pps(x):
    """a prime-power list [(p, e)] (or an index m) as ([(p, e)], the ctypes array, its length)"""
    pps = factor_pps(int(x)) if isinstance(x, (int, np.integer)) else [(int(p), int(e)) for p, e in x]
    arr = (_PP * max(1, len(pps)))()
    for i, (p, e) in enumerate(pps):
        arr[i].prime, arr[i].exponent = p, e
    return pps, arr, len(pps)


def _totient(pps):
    n = 1
    for p, e in pps:
        n *= (p - 1) * p ** (e - 1)
    return n


def crtSetDec(pps_m, pps_m2, p):
    """crtSetDec (CPP/Extension.hs:143-164) on the host: the mod-p CRT set of O_m'/O_m as [K][phi(m')] residues in
    [0, p), decoding basis of O_m'.  pps_m, pps_m2: prime-power lists [(p, e)] or the indices themselves; p: a prime
    that does not divide m'.  Order and root of unity: include/lolhip.h."""
    (_, a, na), (pps2, b, nb) = _pps(pps_m), _pps(pps_m2)
    L = lib()
    K = L.lolhip_crtset_dec(a, na, b, nb, int(p), None, 0)
    _check(min(K, 0), f"crtSetDec(p={p})")
    out = np.zeros((K, _totient(pps2)), dtype=np.int64)
    _check(min(L.lolhip_crtset_dec(a, na, b, nb, int(p), out.ctypes.data_as(_i64p), K), 0), f"crtSetDec(p={p})")
    return out


def crtSet(pps_m, pps_m2, p, e, host=False, stream=None):
    """crtSet (UCyc.hs:540-565): the mod-p^e CRT set of O_m'/O_m as [K][phi(m')] residues in [0, p^e), powerful basis
    of O_m'.  On the device (a CUDA tensor; lolhip_crtset over a plan of the p-free part of m' mod the NTT prime of
    lolhip_crtset_modulus), or with host=True by schoolbook products on the host (numpy; small indices)."""
    (_, a, na), (pps2, b, nb) = _pps(pps_m), _pps(pps_m2)
    L, n2 = lib(), _totient(pps2)
    if host:
        K = L.lolhip_crtset_host(a, na, b, nb, int(p), int(e), None, 0)
        _check(min(K, 0), f"crtSet(p={p}, e={e})")
        out = np.zeros((K, n2), dtype=np.int64)
        _check(min(L.lolhip_crtset_host(a, na, b, nb, int(p), int(e), out.ctypes.data_as(_i64p), K), 0), "crtSet")
        return out
    import torch
    if all(q[0] == int(p) for q in pps2):
        # m' is a power of p: its p-free part is the index 1, the set is {1}; nothing to run on the device
        return torch.from_numpy(crtSet(pps_m, pps_m2, p, e, host=True)).cuda()
    Q = L.lolhip_crtset_modulus(b, nb, int(p), int(e))
    _check(min(Q, 0), f"crtSet(p={p}, e={e})")
    plan = Plan([q for q in pps2 if q[0] != int(p)], [Q])
    K = L.lolhip_crtset(plan._h, a, na, b, nb, int(p), int(e), None, None, 0)          # the statuses and the count
    _check(min(K, 0), f"crtSet(p={p}, e={e})")
    out = torch.empty((K, n2), dtype=torch.int64, device="cuda")
    _check(min(L.lolhip_crtset(plan._h, a, na, b, nb, int(p), int(e), _stream(stream), _devptr(out), K), 0), "crtSet")
    return out


def rqproduct_write(m: int, qs, xs) -> bytes:
    """Serialise decoding-basis residues xs [n][T] as a Lol `RqProduct` message (lol/Lol.proto;
    IZipVector.hs:127-205): one Rq per modulus, centred lifts, unpacked sint64."""
    xs = np.ascontiguousarray(xs, dtype=np.int64)
    qa = np.ascontiguousarray(qs, dtype=np.int64)
    T = len(qa)
    n = xs.size // max(T, 1)
    L = lib()
    need = L.lolhip_rqproduct_write(m, qa.ctypes.data_as(_i64p), T, xs.ctypes.data_as(_i64p), n, None, 0)
    _check(min(need, 0))
    buf = (C.c_uint8 * max(need, 1))()
    wrote = L.lolhip_rqproduct_write(m, qa.ctypes.data_as(_i64p), T, xs.ctypes.data_as(_i64p), n, buf, need)
    _check(min(wrote, 0))
    return bytes(buf[:wrote])


def rqproduct_read(data: bytes):
    """Parse a Lol `RqProduct` message -> (m, [q_t], xs [n][T]) with canonical residues."""
    L = lib()
    raw = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data if data else b"\0")
    m, T = C.c_uint32(0), C.c_int(0)
    qs = np.zeros(16, dtype=np.int64)
    n = L.lolhip_rqproduct_read(raw, len(data), C.byref(m), qs.ctypes.data_as(_i64p), 16, C.byref(T), None, 0)
    _check(min(n, 0))
    xs = np.zeros((n, T.value), dtype=np.int64)
    n2 = L.lolhip_rqproduct_read(raw, len(data), C.byref(m), qs.ctypes.data_as(_i64p), 16, C.byref(T),
                                 xs.ctypes.data_as(_i64p), xs.size)
    _check(min(n2, 0))
    return int(m.value), [int(q) for q in qs[:T.value]], xs


def kshint_read(data: bytes):
    """Parse a SymmSHE `KSHint` message (lol-apps/SHE.proto) -> (m, [q_t], xs [L][K][n][T]),
    decoding basis; `plan.crt(plan.l(xs.reshape(L*K, n, T)))` is the hint slab of keySwitch."""
    L_ = lib()
    raw = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data if data else b"\0")
    m, T, Lh, K = C.c_uint32(0), C.c_int(0), C.c_int(0), C.c_int(0)
    qs = np.zeros(16, dtype=np.int64)
    args = (raw, len(data), C.byref(m), qs.ctypes.data_as(_i64p), 16, C.byref(T), C.byref(Lh), C.byref(K))
    n = L_.lolhip_kshint_read(*args, None, 0)
    _check(min(n, 0))
    xs = np.zeros((Lh.value, K.value, n, T.value), dtype=np.int64)
    _check(min(L_.lolhip_kshint_read(*args, xs.ctypes.data_as(_i64p), xs.size), 0))
    return int(m.value), [int(q) for q in qs[:T.value]], xs


def _raw(data: bytes):
    return (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data if data else b"\0")


def r_read(data: bytes):
    """Lol.proto `R` -> (m, xs[n]) integer decoding-basis coefficients."""
    L_ = lib()
    raw, m = _raw(data), C.c_uint32(0)
    n = L_.lolhip_r_read(raw, len(data), C.byref(m), None, 0)
    _check(min(n, 0))
    xs = np.zeros(n, dtype=np.int64)
    _check(min(L_.lolhip_r_read(raw, len(data), C.byref(m), xs.ctypes.data_as(_i64p), n), 0))
    return int(m.value), xs


def secretkey_read(data: bytes):
    """SHE.proto `SecretKey` -> (m, scaled variance v, sk[n])."""
    L_ = lib()
    raw, m, v = _raw(data), C.c_uint32(0), C.c_double(0)
    n = L_.lolhip_secretkey_read(raw, len(data), C.byref(m), C.byref(v), None, 0)
    _check(min(n, 0))
    xs = np.zeros(n, dtype=np.int64)
    _check(min(L_.lolhip_secretkey_read(raw, len(data), C.byref(m), C.byref(v), xs.ctypes.data_as(_i64p), n), 0))
    return int(m.value), float(v.value), xs


def kqproduct_read(data: bytes):
    """Lol.proto `KqProduct` -> (m, [q_t], xs [n][T] float64)."""
    L_ = lib()
    raw, m, T = _raw(data), C.c_uint32(0), C.c_int(0)
    qs = np.zeros(16, dtype=np.int64)
    n = L_.lolhip_kqproduct_read(raw, len(data), C.byref(m), qs.ctypes.data_as(_i64p), 16, C.byref(T), None, 0)
    _check(min(n, 0))
    xs = np.zeros((n, T.value), dtype=np.float64)
    _check(min(L_.lolhip_kqproduct_read(raw, len(data), C.byref(m), qs.ctypes.data_as(_i64p), 16, C.byref(T),
                                        xs.ctypes.data_as(C.POINTER(C.c_double)), xs.size), 0))
    return int(m.value), [int(q) for q in qs[:T.value]], xs


def linearrq_read(data: bytes):
    """Lol.proto `LinearRq` -> (e, r, m_out, [q_t], xs [C][n][T]) decoding basis, canonical residues."""
    L_ = lib()
    raw = _raw(data)
    e, r, m, Cn, T = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_int(0), C.c_int(0)
    qs = np.zeros(16, dtype=np.int64)
    args = (raw, len(data), C.byref(e), C.byref(r), C.byref(Cn), C.byref(m), qs.ctypes.data_as(_i64p), 16, C.byref(T))
    n = L_.lolhip_linearrq_read(*args, None, 0)
    _check(min(n, 0))
    xs = np.zeros((Cn.value, n, T.value), dtype=np.int64)
    _check(min(L_.lolhip_linearrq_read(*args, xs.ctypes.data_as(_i64p), xs.size), 0))
    return int(e.value), int(r.value), int(m.value), [int(q) for q in qs[:T.value]], xs


def kshint_write(m: int, qs, xs, gad=(0, 0)) -> bytes:
    """xs [L][K][n][T] decoding-basis residues -> SHE.proto `KSHint` bytes (gad = TypeRep words)."""
    xs = np.ascontiguousarray(xs, dtype=np.int64)
    Lh, K, n, T = xs.shape
    qa = np.ascontiguousarray(qs, dtype=np.int64)
    L_ = lib()
    args = (m, qa.ctypes.data_as(_i64p), T, Lh, K, xs.ctypes.data_as(_i64p), n, int(gad[0]), int(gad[1]))
    need = L_.lolhip_kshint_write(*args, None, 0)
    _check(min(need, 0))
    buf = (C.c_uint8 * max(need, 1))()
    wrote = L_.lolhip_kshint_write(*args, buf, need)
    _check(min(wrote, 0))
    return bytes(buf[:wrote])


def tunnelhint_read(data: bytes):
    """SHE.proto `TunnelHint` -> dict(e, r, s, p, func = linearrq_read(...), hints = [kshint_read(...)])."""
    L_ = lib()
    raw = _raw(data)
    e, r, s, p = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    fo, fl = C.c_int64(0), C.c_int64(0)
    nh = L_.lolhip_tunnelhint_read(raw, len(data), C.byref(e), C.byref(r), C.byref(s), C.byref(p), C.byref(fo), C.byref(fl), None, None, 0)
    _check(min(nh, 0))
    ho, hl = np.zeros(max(nh, 1), dtype=np.int64), np.zeros(max(nh, 1), dtype=np.int64)
    _check(min(L_.lolhip_tunnelhint_read(raw, len(data), C.byref(e), C.byref(r), C.byref(s), C.byref(p), C.byref(fo), C.byref(fl),
                                         ho.ctypes.data_as(_i64p), hl.ctypes.data_as(_i64p), nh), 0))
    return {"e": int(e.value), "r": int(r.value), "s": int(s.value), "p": int(p.value),
            "func": linearrq_read(data[fo.value: fo.value + fl.value]),
            "hints": [kshint_read(data[int(o): int(o) + int(l)]) for o, l in zip(ho[:nh], hl[:nh])]}


def _two_pass(fn, *args) -> bytes:
    """size query (out = NULL), then the write"""
    need = fn(*args, None, 0)
    _check(min(need, 0))
    buf = (C.c_uint8 * max(need, 1))()
    wrote = fn(*args, buf, need)
    _check(min(wrote, 0))
    return bytes(buf[:wrote])


def _byte_parts(parts):
    """list of bytes objects -> (array of pointers, array of lengths, keep-alive list)"""
    keep = [(C.c_uint8 * max(len(p), 1)).from_buffer_copy(p if p else b"\0") for p in parts]
    ptrs = (C.POINTER(C.c_uint8) * max(len(parts), 1))(*[C.cast(k, C.POINTER(C.c_uint8)) for k in keep])
    lens = np.array([len(p) for p in parts] or [0], dtype=np.int64)
    return ptrs, lens, keep


def r_write(m: int, xs) -> bytes:
    """integer decoding-basis coefficients xs [n] -> Lol.proto `R` bytes."""
    xs = np.ascontiguousarray(xs, dtype=np.int64)
    return _two_pass(lib().lolhip_r_write, m, xs.ctypes.data_as(_i64p), xs.size)


def secretkey_write(m: int, v: float, xs) -> bytes:
    """SHE.proto `SecretKey` (ring element xs [n] as `R`, scaled variance v)."""
    xs = np.ascontiguousarray(xs, dtype=np.int64)
    return _two_pass(lib().lolhip_secretkey_write, m, C.c_double(v), xs.ctypes.data_as(_i64p), xs.size)


def linearrq_write(e: int, r: int, m: int, qs, xs) -> bytes:
    """xs [C][n][T] (values of an E-linear function on the relative decoding basis) -> Lol.proto `LinearRq` bytes."""
    xs = np.ascontiguousarray(xs, dtype=np.int64)
    Cn, n, T = xs.shape
    qa = np.ascontiguousarray(qs, dtype=np.int64)
    return _two_pass(lib().lolhip_linearrq_write, e, r, m, qa.ctypes.data_as(_i64p), T, Cn, xs.ctypes.data_as(_i64p), n)


def tunnelhint_write(func: bytes, hints, e: int, r: int, s: int, p: int) -> bytes:
    """SHE.proto `TunnelHint` from an encoded LinearRq and a list of encoded KSHints."""
    fbuf = (C.c_uint8 * max(len(func), 1)).from_buffer_copy(func if func else b"\0")
    ptrs, lens, keep = _byte_parts(list(hints))
    return _two_pass(lib().lolhip_tunnelhint_write, fbuf, len(func), ptrs, lens.ctypes.data_as(_i64p), len(hints), e, r, s, p)


def chain_write(elems) -> bytes:
    """HomomPRF.proto chain (LinearFuncChain / TunnelHintChain / RoundHintChain) of encoded elements."""
    ptrs, lens, keep = _byte_parts(list(elems))
    return _two_pass(lib().lolhip_chain_write, ptrs, lens.ctypes.data_as(_i64p), len(elems))


def chain_read(data: bytes):
    """HomomPRF.proto chain -> list of the encoded elements (hand them to linearrq_read / tunnelhint_read / kshint_read)."""
    L_ = lib()
    raw = _raw(data)
    cnt = L_.lolhip_chain_read(raw, len(data), None, None, 0)
    _check(min(cnt, 0))
    off, ln = np.zeros(max(cnt, 1), dtype=np.int64), np.zeros(max(cnt, 1), dtype=np.int64)
    _check(min(L_.lolhip_chain_read(raw, len(data), off.ctypes.data_as(_i64p), ln.ctypes.data_as(_i64p), cnt), 0))
    return [data[int(o): int(o) + int(l)] for o, l in zip(off[:cnt], ln[:cnt])]


def _np(a):
    a = np.ascontiguousarray(a, dtype=np.int64)
    return a, a.ctypes.data_as(_i64p)


def _devptr(x):
    """raw device address of a torch CUDA int64 tensor, or an int address"""
    if isinstance(x, int):
        return x
    if not (x.is_cuda and x.is_contiguous() and x.dtype.__str__() == "torch.int64"):
        raise TypeError("expected a contiguous int64 CUDA tensor")
    return x.data_ptr()


def _stream(stream):
    if stream is None:
        try:
            import torch
            if torch.cuda.is_available():
                return torch.cuda.current_stream().cuda_stream
        except ImportError:
            pass
        return 0
    return int(stream)


class Plan:
    """Twiddles, g vectors, stage programs and moduli for one (m, moduli), resident in HBM.

    Mirrors what lol-cpp's shim marshals per call: `ru`/`ruInv` (CPP.hs:422-442),
    `mhatInv` (ZqBasic.hs:167-171), `gCRT`/`gInvCRT` (CPP.hs:444-454), the prime-power
    list (CPP.hs:325-337) and the moduli (Backend.hs:195-199)."""

    def __init__(self, pps, qs, host_only=False, omega_pp=None, mhatinv=None):
        self.pps = [(int(p), int(e)) for p, e in pps]
        self.qs = [int(q) for q in qs]
        self.host_only = bool(host_only)
        arr = (_PP * max(1, len(self.pps)))()
        for i, (p, e) in enumerate(self.pps):
            arr[i].prime, arr[i].exponent = p, e
        qa = (C.c_int64 * len(self.qs))(*self.qs)
        h = C.c_void_p()
        L = lib()
        if omega_pp is None and mhatinv is None:
            rc = L.lolhip_plan_create(arr, len(self.pps), qa, len(self.qs), int(host_only), C.byref(h))
        else:
            om = None if omega_pp is None else (C.c_int64 * len(omega_pp))(*[int(v) for v in omega_pp])
            mh = None if mhatinv is None else (C.c_int64 * len(mhatinv))(*[int(v) for v in mhatinv])
            rc = L.lolhip_plan_create_roots(arr, len(self.pps), qa, len(self.qs), om, mh, int(host_only), C.byref(h))
        _check(rc, f"plan_create(pps={self.pps}, qs={self.qs})")
        self._h = h
        self.n = int(L.lolhip_plan_n(h))
        self.m = int(L.lolhip_plan_m(h))
        self.T = int(L.lolhip_plan_T(h))
        self.has_crt = bool(L.lolhip_plan_has_crt(h))

    @classmethod
    def for_index(cls, m, qs, **kw):
        return cls(factor_pps(m), qs, **kw)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.lolhip_plan_destroy(h)

    # ---- tables -------------------------------------------------------------------
    def _table(self, which, k=0):
        L = lib()
        cnt = L.lolhip_plan_table(self._h, which, k, None, 0)
        out = np.zeros(cnt, dtype=np.int64)
        if cnt:
            L.lolhip_plan_table(self._h, which, k, out.ctypes.data_as(_i64p), cnt)
        return out

    def ru(self, k): return self._table(0, k)
    def ruInv(self, k): return self._table(1, k)
    def mhatInv(self): return self._table(2)
    def gCRT(self): return self._table(3).reshape(self.n, self.T)
    def gInvCRT(self): return self._table(4).reshape(self.n, self.T)

    def liftConsts(self):
        """Constants of the lift to the integers (errorTerm / decrypt): dict of `pinv` [T] ((q_0...q_(i-1))^-1 mod q_i),
        `qmod` [T][T] (qmod[i][j] = q_j mod q_i) and `half` [T] (mixed-radix digits of floor((Q-1)/2))."""
        t, T = self._table(12), self.T
        return {"pinv": t[:T], "qmod": t[T:T + T * T].reshape(T, T), "half": t[T + T * T:]}

    def program(self, inverse=False, polymul=False):
        """Stage program a lone crt / crtInv launches (inspection): rows (kind, prime or first level, length or levels,
        stride).  polymul=True: the forward / inverse program of the one-launch poly-mul (no rows when poly-mul is composed
        of lone transforms)."""
        return self._table((13 if polymul else 10) + (1 if inverse else 0)).reshape(-1, 4)

    # ---- helpers ------------------------------------------------------------------
    def _batch(self, a):
        per = self.n * self.T
        if a.size % per:
            raise ValueError(f"array of {a.size} residues is not a whole number of [n={self.n}, T={self.T}] polynomials")
        return a.size // per

    def _host(self, op, y, b=None):
        y, yp = _np(y)
        y = y.copy()
        yp = y.ctypes.data_as(_i64p)
        B = self._batch(y)
        bp = None
        if b is not None:
            b, bp = _np(b)
            if b.size != y.size:
                raise ValueError("operand shapes differ")
        rc = lib().lolhip_op_host(self._h, op, yp, bp, B)
        if rc == ERR_NOT_DIVISIBLE:
            return None
        _check(rc)
        return y

    def _dev(self, name, y, stream):
        B = self._batch_t(y)
        rc = getattr(lib(), f"lolhip_{name}_batch")(self._h, _stream(stream), _devptr(y), B)
        if rc == ERR_NOT_DIVISIBLE:
            return None
        _check(rc)
        return y

    def _batch_t(self, t):
        per = self.n * self.T
        numel = t.numel()
        if numel % per:
            raise ValueError("tensor is not a whole number of polynomials")
        return numel // per

    def _op(self, op, name, y, stream=None):
        if isinstance(y, np.ndarray) or isinstance(y, (list, tuple)):
            return self._host(op, y)
        return self._dev(name, y, stream)

    # ---- the Tensor interface (in place for device tensors, copies for numpy) -----
    def crt(self, y, stream=None): return self._op(OP_CRT, "crt", y, stream)
    def crtInv(self, y, stream=None): return self._op(OP_CRTINV, "crtinv", y, stream)
    def l(self, y, stream=None): return self._op(OP_L, "l", y, stream)
    def lInv(self, y, stream=None): return self._op(OP_LINV, "linv", y, stream)
    def mulGPow(self, y, stream=None): return self._op(OP_MULGPOW, "mulgpow", y, stream)
    def mulGDec(self, y, stream=None): return self._op(OP_MULGDEC, "mulgdec", y, stream)
    def divGPow(self, y, stream=None): return self._op(OP_DIVGPOW, "divgpow", y, stream)
    def divGDec(self, y, stream=None): return self._op(OP_DIVGDEC, "divgdec", y, stream)
    def mulGCRT(self, y, stream=None): return self._op(OP_MULGCRT, "mulgcrt", y, stream)
    def divGCRT(self, y, stream=None): return self._op(OP_DIVGCRT, "divgcrt", y, stream)

    def mul(self, a, b, stream=None):
        """zipWithT (*): a * b pointwise (a is overwritten when it is a device tensor)."""
        if isinstance(a, np.ndarray):
            return self._host(OP_MUL, a, b)
        _check(lib().lolhip_mul_batch(self._h, _stream(stream), _devptr(a), _devptr(b), self._batch_t(a)))
        return a

    def polymul(self, a, b, out=None, stream=None):
        """crtInv(crt a * crt b): one ring product per batch item, powerful basis in and out."""
        if isinstance(a, np.ndarray):
            return self._host(OP_POLYMUL, a, b)
        out = a if out is None else out
        _check(lib().lolhip_polymul_batch(self._h, _stream(stream), _devptr(out), _devptr(a), _devptr(b), self._batch_t(a)))
        return out


    # ---- floating-point members: float64, tolerance contract -----------
    def _float_op(self, name, y, complex_):
        """numpy in -> numpy out (staged through HBM); torch CUDA tensor -> in place."""
        import torch
        host = isinstance(y, np.ndarray)
        want = torch.complex128 if complex_ else torch.float64
        t = torch.from_numpy(np.ascontiguousarray(y, dtype=np.complex128 if complex_ else np.float64)).cuda() if host else y
        if not (t.is_cuda and t.is_contiguous() and t.dtype == want):
            raise TypeError(f"expected a contiguous {want} CUDA tensor")
        if t.numel() % self.n:
            raise ValueError("tensor is not a whole number of polynomials")
        _check(getattr(lib(), f"lolhip_{name}_batch")(self._h, _stream(None), t.data_ptr(), t.numel() // self.n))
        return t.cpu().numpy() if host else t

    def crtC(self, y):
        """CRT over C (tensorCRTC, crt.cpp:583-586): complex128 [..., n]."""
        return self._float_op("crtc", y, True)

    def crtInvC(self, y):
        """inverse CRT over C including mhat^-1 (tensorCRTInvC, crt.cpp:589-598)."""
        return self._float_op("crtinvc", y, True)

    def gaussianDec(self, y):
        """iid real Gaussians [..., n] -> decoding-basis sample (tensorGaussianDec, random.cpp:61-64)."""
        return self._float_op("gaussian_dec", y, False)

    # ---- l, lInv, mulG, divG over Z, R and C ------------------------------
    _ELT = {"int64": ELT_I64, "float64": ELT_F64, "complex128": ELT_C64}

    def eltOp(self, op, y, T=None, stream=None):
        """One of OP_L, OP_LINV, OP_MULGPOW, OP_MULGDEC, OP_DIVGPOW, OP_DIVGDEC over a slab [..., n, T] of int64 (arithmetic
        mod 2^64), float64 or complex128 elements (tensorL{R,Double,C}, tensorLInv*, tensorG*{R,C}; lolhip_elt_op_batch).  The
        plan's moduli play no role.  T: components per coefficient; by default the last axis when the one before it has
        length n, else 1.  numpy in -> numpy out (staged through HBM); a torch CUDA tensor is transformed in place.  Returns
        y, or (y, ok) for divG over int64: ok int32 [B], 1 where item b was divisible by g (it then holds the quotient; an
        item with ok = 0 holds the undivided transform)."""
        import torch
        host = isinstance(y, np.ndarray)
        elt = self._ELT.get(str(y.dtype).replace("torch.", ""))
        if elt is None:
            raise TypeError("expected an int64, float64 or complex128 array or CUDA tensor")
        if T is None:
            T = int(y.shape[-1]) if len(y.shape) >= 2 and y.shape[-2] == self.n else 1
        # a dry run at B = 0: every host status is raised before anything is staged
        _check(lib().lolhip_elt_op_batch(self._h, None, int(op), elt, int(T), None, None, 0), "elt_op")
        t = torch.from_numpy(np.ascontiguousarray(y)).cuda() if host else y
        if not (t.is_cuda and t.is_contiguous()):
            raise TypeError("expected a contiguous CUDA tensor")
        if t.numel() % (self.n * T):
            raise ValueError(f"slab is not a whole number of [n={self.n}, T={T}] polynomials")
        B = t.numel() // (self.n * T)
        divi = elt == ELT_I64 and op in (OP_DIVGPOW, OP_DIVGDEC)
        ok = torch.empty((max(B, 1),), dtype=torch.int32, device=t.device)[:B] if divi else None
        _check(lib().lolhip_elt_op_batch(self._h, _stream(stream), int(op), elt, T, t.data_ptr(),
                                         ok.data_ptr() if divi else None, B), "elt_op")
        if divi:
            return (t.cpu().numpy(), ok.cpu().numpy()) if host else (t, ok)
        return t.cpu().numpy() if host else t

    def lR(self, y, T=None, stream=None): return self.eltOp(OP_L, y, T, stream)
    def lInvR(self, y, T=None, stream=None): return self.eltOp(OP_LINV, y, T, stream)
    def mulGPowR(self, y, T=None, stream=None): return self.eltOp(OP_MULGPOW, y, T, stream)
    def mulGDecR(self, y, T=None, stream=None): return self.eltOp(OP_MULGDEC, y, T, stream)
    def divGPowR(self, y, T=None, stream=None): return self.eltOp(OP_DIVGPOW, y, T, stream)
    def divGDecR(self, y, T=None, stream=None): return self.eltOp(OP_DIVGDEC, y, T, stream)

    # ---- ring-level pipelines of SymmSHE (include/lolhip.h) -----------
    # numpy in -> numpy out (staged through HBM with torch); CUDA tensors in -> CUDA tensors out.
    @staticmethod
    def _stage(*arrays):
        import torch
        host = isinstance(arrays[0], np.ndarray)
        dev = [None if a is None else (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda() if host else a)
               for a in arrays]
        return host, dev

    @staticmethod
    def _unstage(host, *tensors):
        out = tuple(t.cpu().numpy() if host else t for t in tensors)
        return out if len(out) > 1 else out[0]

    @staticmethod
    def _run_staged(call, stream, inputs, B, work_len, out_shape, out=None):
        """The protocol of the batched SymmSHE entries.  call(stream, ptrs, out, work, B) wraps one C entry: first a dry
        run at B = 0 with null pointers, so every host status is raised before anything touches the device; then numpy
        inputs (inputs[0] decides) are staged, the work buffer (work_len() words, at least one) and the output
        (out_shape(), unless `out` is given) allocated, the real call made and the output unstaged."""
        import torch
        _check(call(None, [None] * len(inputs), None, None, 0))
        host = isinstance(inputs[0], np.ndarray)
        if host:
            _, inputs = Plan._stage(*inputs)
        dev = inputs[0].device
        wl = work_len()
        _check(min(wl, 0))
        work = torch.empty((max(wl, 1),), dtype=torch.int64, device=dev)
        if out is None:
            out = torch.empty(out_shape(), dtype=torch.int64, device=dev)
        _check(call(_stream(stream), [_devptr(t) for t in inputs], _devptr(out), _devptr(work), B))
        return Plan._unstage(host, out)

    def ctMulCRT(self, c0, c1, d0, d1, stream=None):
        """(g c0 d0, g (c0 d1 + c1 d0), g c1 d1): mulG <$> c*d for two linear ciphertexts, every
        operand in the CRT basis (SymmSHE.hs:444-449)."""
        import torch
        host, (c0, c1, d0, d1) = self._stage(c0, c1, d0, d1)
        e = [torch.empty_like(c0) for _ in range(3)]
        _check(lib().lolhip_ctmul_crt_batch(self._h, _stream(stream), *map(_devptr, (c0, c1, d0, d1, *e)), self._batch_t(c0)))
        return self._unstage(host, *e)

    def decomposeLen(self, base):
        L = lib().lolhip_decompose_len(self._h, int(base))
        _check(min(L, 0))
        return L

    def gadget(self, base):
        """gadget vector [L][T] (Gadget.hs:92-94 over ZqBasic.hs:227-229,248-253)."""
        L = self.decomposeLen(base)
        out = np.zeros((L, self.T), dtype=np.int64)
        _check(min(lib().lolhip_gadget(self._h, int(base), out.ctypes.data_as(_i64p), out.size), 0))
        return out

    def decompose(self, c, base, stream=None):
        """powerful-basis c [B][n][T] -> reduced digit polynomials [L][B][n][T] (Cyc.hs:592-604)."""
        import torch
        host, (c,) = self._stage(c)
        B, L = self._batch_t(c), self.decomposeLen(base)
        out = torch.empty((L, B, self.n, self.T), dtype=torch.int64, device=c.device)
        _check(lib().lolhip_decompose_batch(self._h, _stream(stream), _devptr(c), int(base), _devptr(out), B))
        return self._unstage(host, out)

    _BASIS = {"dec": 0, "pow": 1, "crt": 2, 0: 0, 1: 1, 2: 2}

    def gadgetEncode(self, s, base, e=None, stream=None):
        """Gadget.encode plus noise (Gadget.hs:47-56): out_j = g_j s + reduce (e_j) for s [B][n][T] and integer errors
        e [L][B][n] (None: no noise) -> [L][B][n][T], L = decomposeLen(base); s and e in one basis, any."""
        import torch
        _check(lib().lolhip_gadget_encode_batch(self._h, None, None, int(base), None, None, 0))
        host, (s, e) = self._stage(s, e)
        B, L = self._batch_t(s), self.decomposeLen(base)
        if e is not None and e.numel() != L * B * self.n:
            raise ValueError(f"errors are not [L={L}][B={B}][n={self.n}]")
        out = torch.empty((L, B, self.n, self.T), dtype=torch.int64, device=s.device)
        _check(lib().lolhip_gadget_encode_batch(self._h, _stream(stream), _devptr(s), int(base),
                                                None if e is None else _devptr(e), _devptr(out), B))
        return self._unstage(host, out)

    def gadgetCorrectWorkLen(self, base, basis="dec", B=1):
        wl = lib().lolhip_gadget_correct_work_len(self._h, int(base), self._BASIS[basis], int(B))
        _check(min(wl, 0))
        return wl

    def gadgetCorrect(self, xs, base, basis="dec", errors=True, stream=None):
        """Gadget error correction (Correct gad (Cyc t m zq), Cyc.hs:615-621): xs [L][B][n][T], the noisy multiples
        g_j s + e_j in `basis` ("dec", "pow" or "crt") -> (u [B][n][T], es [L][B][n] int64), both in the decoding basis;
        es is None with errors=False.  T = 1 or 2; defined for every input."""
        import torch
        L, bs = self.decomposeLen(base), self._BASIS[basis]
        lb = lib()
        _check(lb.lolhip_gadget_correct_batch(self._h, None, None, int(base), bs, None, None, None, 0))
        host, (xs,) = self._stage(xs)
        if self._batch_t(xs) % L:
            raise ValueError(f"xs is not [L={L}][B][n={self.n}][T={self.T}]")
        B = self._batch_t(xs) // L
        wl = self.gadgetCorrectWorkLen(base, basis, B)
        work = torch.empty((max(wl, 1),), dtype=torch.int64, device=xs.device)
        u = torch.empty((B, self.n, self.T), dtype=torch.int64, device=xs.device)
        es = torch.empty((L, B, self.n), dtype=torch.int64, device=xs.device) if errors else None
        _check(lb.lolhip_gadget_correct_batch(self._h, _stream(stream), _devptr(xs), int(base), bs, _devptr(u),
                                              None if es is None else _devptr(es), _devptr(work), B))
        if es is None:
            return self._unstage(host, u), None
        return self._unstage(host, u, es)

    def knapsack(self, xs_crt, hint, addend=None, stream=None):
        """sum_j xs_j *>> hint_j (+ addend), CRT basis (SymmSHE.hs:302-304): xs [L][B][n][T],
        hint [L][K][n][T] -> [K][B][n][T]."""
        import torch
        host, (xs_crt, hint, addend) = self._stage(xs_crt, hint, addend)
        L, K = xs_crt.shape[0], hint.shape[1]
        B = self._batch_t(xs_crt) // max(L, 1)
        out = torch.empty((K, B, self.n, self.T), dtype=torch.int64, device=hint.device)
        _check(lib().lolhip_knapsack_batch(self._h, _stream(stream), _devptr(xs_crt), L, _devptr(hint), K,
                                           None if addend is None else _devptr(addend), _devptr(out), B))
        return self._unstage(host, out)

    def keySwitch(self, c2_pow, base, hint, addend=None, stream=None):
        """addend + knapsack hint (crt (reduce <$> decompose c2)) — `switch`, SymmSHE.hs:312-314."""
        import torch
        host, (c2_pow, hint, addend) = self._stage(c2_pow, hint, addend)
        B, L, K = self._batch_t(c2_pow), self.decomposeLen(base), hint.shape[1]
        work = torch.empty((L, B, self.n, self.T), dtype=torch.int64, device=c2_pow.device)
        out = torch.empty((K, B, self.n, self.T), dtype=torch.int64, device=c2_pow.device)
        _check(lib().lolhip_keyswitch_batch(self._h, _stream(stream), _devptr(c2_pow), int(base), _devptr(hint), K,
                                            None if addend is None else _devptr(addend), _devptr(out), _devptr(work), B))
        return self._unstage(host, out)

    def rescaleDropFirst(self, c, stream=None):
        """RescaleCyc (a,b) -> b (Cyc.hs:529-542): [B][n][T] -> [B][n][T-1]."""
        import torch
        host, (c,) = self._stage(c)
        B = self._batch_t(c)
        out = torch.empty((B, self.n, self.T - 1), dtype=torch.int64, device=c.device)
        _check(lib().lolhip_rescale_drop_batch(self._h, _stream(stream), _devptr(c), _devptr(out), B))
        return self._unstage(host, out)

    # ---- errorTerm / decrypt (lol-apps SymmSHE.hs:153-178) ------------------------------
    @staticmethod
    def _enc(enc):
        return {"LSD": 0, "MSD": 1, 0: 0, 1: 1}[enc]

    def errorTerm(self, cs, s_crt, p, enc="LSD", cs_crt=False, stream=None):
        """liftCyc Dec (evaluate c s) after toLSD (SymmSHE.hs:153-157): ciphertext components cs (a list of [B][n][T]
        or one [ncs][B][n][T] array; powerful basis, or CRT basis with cs_crt), secret key s_crt [n][T] in the CRT
        basis -> [B][n] int64 centred lifts mod Q (INT64_MIN where the lift does not fit)."""
        L = lib()
        _, cs, ncs, B = self._cs(cs)
        e = self._enc(enc)
        return self._run_staged(
            lambda st, i, o, w, b: L.lolhip_error_term_batch(self._h, st, i[0], ncs, int(cs_crt), i[1], e, int(p), o, w, b),
            stream, (cs, s_crt), B, lambda: L.lolhip_decrypt_work_len(self._h, ncs, B), lambda: (B, self.n))

    def decrypt(self, cs, s_crt, pp, ext=None, enc="LSD", k=0, l=1, cs_crt=False, stream=None):
        """SymmSHE decrypt (SymmSHE.hs:169-174): l' twace (divG^k (reduce_p (errorTerm))).  pp: the Plan of index m' over
        the plaintext modulus p alone; ext: an Ext from the Plan of (m, p) to pp, or None for m = m'.  Returns [B][n_m]
        residues mod p in the powerful basis of R_m."""
        L = lib()
        _, cs, ncs, B = self._cs(cs)
        e, xh = self._enc(enc), (None if ext is None else ext._h)
        n_out = pp.n if ext is None else ext.lo.n
        return self._run_staged(
            lambda st, i, o, w, b: L.lolhip_decrypt_batch(self._h, pp._h, xh, st, i[0], ncs, int(cs_crt), i[1], e, int(k),
                                                           int(l), o, w, b),
            stream, (cs, s_crt), B, lambda: L.lolhip_decrypt_work_len(self._h, ncs, B), lambda: (B, n_out))

    # ---- encrypt / genSK (lol-apps SymmSHE.hs:120-146) -------------------------------------
    @staticmethod
    def _key(key):
        key = os.urandom(32) if key is None else bytes(key)
        if len(key) != 32:
            raise ValueError("key must be 32 bytes")
        return key

    def encrypt(self, pt, s_crt, pp, svar, key=None, ctr=0, ext=None, out_crt=False, stream=None):
        """SymmSHE encrypt (SymmSHE.hs:138-146) of B plaintexts pt [B][n_m] (in (-p, p), powerful basis of R_m) under
        the key s_crt [n][T] (CRT basis) -> [2][B][n][T] = (c0, c1) of CT LSD 0 1, powerful basis or the CRT basis with
        out_crt.  pp: the Plan of index m' over p alone; ext: an Ext from the Plan of (m, p) to pp, or None for m = m'.
        Samples from the ChaCha20 stream of (key, ctr + b) (include/lolhip.h); key None draws a fresh one.  Never reuse
        (key, ctr + b): advance ctr by B between calls."""
        L = lib()
        kb, xh = self._key(key), (None if ext is None else ext._h)
        n_m = pp.n if ext is None else ext.lo.n
        size = pt.size if isinstance(pt, np.ndarray) else pt.numel()
        B = size // max(n_m, 1)
        if B * n_m != size:
            raise ValueError("pt is not [B][n_m]")
        return self._run_staged(
            lambda st, i, o, w, b: L.lolhip_encrypt_batch(self._h, pp._h, xh, st, i[0], i[1], float(svar), kb, int(ctr),
                                                           int(out_crt), o, w, b),
            stream, (pt, s_crt), B, lambda: L.lolhip_encrypt_work_len(self._h, B), lambda: (2, B, self.n, self.T))

    def errorRounded(self, svar, B=1, key=None, ctr=0, stream=None):
        """errorRounded svar (UCyc.hs:422-429; genSK, SymmSHE.hs:120-122): [B][n] int64 decoding-basis coefficients,
        from the ChaCha20 stream of (key, ctr + b); key None draws a fresh one."""
        import torch
        L = lib()
        kb = self._key(key)
        _check(L.lolhip_error_rounded_batch(self._h, None, float(svar), kb, int(ctr), None, None, 0))
        out = torch.empty((int(B), self.n), dtype=torch.int64, device="cuda")
        _check(L.lolhip_error_rounded_batch(self._h, _stream(stream), float(svar), kb, int(ctr), _devptr(out), None, int(B)))
        return out

    # ---- key-switch hints (lol-apps SymmSHE.hs:262-296, 330-355) -------------------------
    def ksHint(self, s_crt, vals_crt, svar, base, key=None, ctr=0, stream=None):
        """ksHint skout val (SymmSHE.hs:286-296) for B values vals_crt [B][n][T] (CRT basis) under the key s_crt [n][T]
        (CRT basis) -> [B][L][2][n][T] CRT-basis hints; [b] is the hint keySwitch takes.  Row j of item b is LWE sample
        ctr + b L + j of the ChaCha20 stream (include/lolhip.h): advance ctr by B L between calls; key None draws a
        fresh key."""
        L = lib()
        kb = self._key(key)
        size = vals_crt.size if isinstance(vals_crt, np.ndarray) else vals_crt.numel()
        per = self.n * self.T
        B = size // per
        if B * per != size:
            raise ValueError("vals_crt is not [B][n][T]")
        return self._run_staged(
            lambda st, i, o, w, b: L.lolhip_kshint_batch(self._h, st, i[1], i[0], float(svar), int(base), kb, int(ctr),
                                                          o, w, b),
            stream, (vals_crt, s_crt), B, lambda: L.lolhip_kshint_work_len(self._h, int(base), B),
            lambda: (B, self.decomposeLen(base), 2, self.n, self.T))

    def ksLinearHint(self, s_out_crt, s_in_crt, svar, base, key=None, ctr=0, stream=None):
        """ksLinearHint skout skin (SymmSHE.hs:330-335) = ksHint skout s_in: one [L][2][n][T] hint."""
        return self.ksHint(s_out_crt, s_in_crt, svar, base, key=key, ctr=ctr, stream=stream)[0]

    def ksQuadCircHint(self, s_crt, svar, base, key=None, ctr=0, stream=None):
        """ksQuadCircHint sk (SymmSHE.hs:352-355) = ksHint sk (s*s), s*s formed on the device: one [L][2][n][T] hint."""
        _check(lib().lolhip_kshint_batch(self._h, None, None, None, float(svar), int(base), self._key(key), int(ctr), None,
                                         None, 0))
        host, (s_crt,) = self._stage(s_crt)
        s2 = s_crt.clone().contiguous()
        self.mul(s2, s_crt, stream=stream)
        return self._unstage(host, self.ksHint(s_crt, s2, svar, base, key=key, ctr=ctr, stream=stream)[0])

    # ---- SymmSHE public operations and ciphertext addition (lol-apps SymmSHE.hs:214-230, 381-436) ---------------
    # A ciphertext is cs ([ncs][B][n][T], or a list of [B][n][T]) with its (enc, k, l); each call takes and returns the
    # parts it changes.  numpy in -> numpy out (staged through HBM); CUDA tensors in -> CUDA tensors out.
    def encodeScales(self, p, to_msd):
        """The encoding factors of the product ring (ZqBasic.hs:132-137, Prelude.hs:310-315): to_msd -> lsdToMSD =
        ([p^-1 mod q_t], -Q mod p), else msdToLSD = ([p mod q_t], (-Q)^-1 mod p).  Host only."""
        zq = np.zeros(self.T, dtype=np.int64)
        zp = C.c_int64(0)
        _check(lib().lolhip_encode_scales(self._h, int(p), int(bool(to_msd)), zq.ctypes.data_as(_i64p), C.byref(zp)))
        return [int(v) for v in zq], int(zp.value)

    def _cs(self, cs):
        """(host?, cs as one [ncs][B][n][T] array or tensor, ncs, B)"""
        import torch
        if isinstance(cs, (list, tuple)):
            host = isinstance(cs[0], np.ndarray)
            cs = np.stack([np.asarray(c, dtype=np.int64) for c in cs]) if host else torch.stack(list(cs))
        host = isinstance(cs, np.ndarray)
        size = cs.size if host else cs.numel()
        ncs = int(cs.shape[0])
        B = size // max(ncs * self.n * self.T, 1)
        if ncs * B * self.n * self.T != size:
            raise ValueError("cs is not [ncs][B][n][T]")
        return host, cs, ncs, B

    def _per_mod(self, v):
        v = [int(v)] * self.T if np.ndim(v) == 0 else [int(x) for x in v]
        if len(v) != self.T:
            raise ValueError("expected one scalar per modulus")
        return (C.c_int64 * self.T)(*v)

    def ctLinComb(self, a, alpha, b=None, beta=None, out=None, stream=None):
        """out_i = alpha_t a_i + beta_t b_i mod q_t, i < max(na, nb), a missing component counting as zero
        (lolhip_ct_lincomb_batch); alpha, beta: an int or one int per modulus.  Either basis; out may be a or b."""
        import torch
        host, a, na, B = self._cs(a)
        nb = 0
        if b is not None:
            _, b, nb, Bb = self._cs(b)
            if Bb != B:
                raise ValueError("batch sizes differ")
        al = self._per_mod(alpha)
        be = self._per_mod(0 if beta is None else beta) if b is not None else None
        L = lib()
        _check(L.lolhip_ct_lincomb_batch(self._h, None, None, na, al, None if b is None else 1, nb, be, None, 0))
        host, (a, b) = self._stage(a, b) if host else (False, (a, b))
        if out is None:
            out = torch.empty((max(na, nb), B, self.n, self.T), dtype=torch.int64, device=a.device)
        _check(L.lolhip_ct_lincomb_batch(self._h, _stream(stream), _devptr(a), na, al, None if b is None else _devptr(b), nb,
                                         be, _devptr(out), B))
        return self._unstage(host, out)

    @staticmethod
    def _decode(v, p):
        """decode' (ZqBasic.hs:92-94): v mod p lifted to [-p/2, p/2)"""
        v = int(v) % int(p)
        return v - p if 2 * v >= p else v

    def toMSD(self, cs, p, enc="LSD", l=1, stream=None):
        """toMSD (SymmSHE.hs:214-222) -> (cs, "MSD", l)"""
        if self._enc(enc) == 1:
            return cs, "MSD", int(l) % p
        zq, zp = self.encodeScales(p, True)
        return self.ctLinComb(cs, zq, stream=stream), "MSD", int(l) * zp % p

    def toLSD(self, cs, p, enc="MSD", l=1, stream=None):
        """toLSD (SymmSHE.hs:224-230) -> (cs, "LSD", l)"""
        if self._enc(enc) == 0:
            return cs, "LSD", int(l) % p
        zq, zp = self.encodeScales(p, False)
        return self.ctLinComb(cs, zq, stream=stream), "LSD", int(l) * zp % p

    def mulScalar(self, cs, a, p, stream=None):
        """mulScalar a (SymmSHE.hs:392-399): every c_i times decode'(a mod p) mod q_t"""
        return self.ctLinComb(cs, self._decode(a, p), stream=stream)

    def ctNegate(self, cs, stream=None):
        """negate (SymmSHE.hs:420-436): every c_i times -1"""
        return self.ctLinComb(cs, -1, stream=stream)

    def mulGCT(self, cs, k, cs_crt=False, stream=None):
        """mulGCT (SymmSHE.hs:413-416): mulG on every c_i (mulGCRT or mulGPow) -> (cs, k + 1)"""
        host, cs, _, _ = self._cs(cs)
        host, (cs,) = self._stage(cs) if host else (False, (cs,))
        y = cs.clone()
        self._dev("mulgcrt" if cs_crt else "mulgpow", y, stream)
        return self._unstage(host, y), int(k) + 1

    def ctAdd(self, ct1, ct2, p, cs_crt=False, stream=None):
        """(+) (SymmSHE.hs:420-436) of ct = (cs, enc, k, l), aligned as the reference does, in order: l1 != l2 ->
        mulScalar (l1 / l2) on ct1; unequal k -> mulGCT on the smaller; unequal encodings -> toMSD of the LSD one; then
        the componentwise sum (the shorter one padded with zeros).  Returns (cs, enc, k, l)."""
        (c1, e1, k1, l1), (c2, e2, k2, l2) = ct1, ct2
        e1, e2, l1, l2 = self._enc(e1), self._enc(e2), int(l1) % p, int(l2) % p
        while True:
            if l1 != l2:
                c1, l1 = self.mulScalar(c1, l1 * pow(l2, -1, p) % p, p, stream=stream), l2
            elif k1 != k2:
                if k1 < k2:
                    c1, k1 = self.mulGCT(c1, k1, cs_crt, stream=stream)
                else:
                    c2, k2 = self.mulGCT(c2, k2, cs_crt, stream=stream)
            elif e1 != e2:
                if e1 == 0:
                    c1, _, l1 = self.toMSD(c1, p, 0, l1, stream=stream)
                    e1 = 1
                else:
                    c2, _, l2 = self.toMSD(c2, p, 0, l2, stream=stream)
                    e2 = 1
            else:
                break
        return self.ctLinComb(c1, 1, c2, 1, stream=stream), ("LSD", "MSD")[e1], k1, l1

    def _public(self, v, n_m, B, stride):
        """public values -> (array or tensor, stride): stride None infers 0 for one value ([n_m] or [1][n_m])"""
        size = v.size if isinstance(v, np.ndarray) else v.numel()
        if stride is None:
            stride = 0 if size == n_m else n_m
        if B > 0 and size < (stride * (B - 1) if stride else 0) + n_m:
            raise ValueError("public values too short for the batch")
        return v, int(stride)

    def addPublic(self, b, cs, p, pp_m=None, ext=None, enc="LSD", k=0, l=1, cs_crt=False, cs_shared=False, stride=None,
                  B=None, stream=None):
        """addPublic b (SymmSHE.hs:381-390): toLSD, then c_0 + embed (decode' (l^-1 g^k b)) -> (cs, "LSD", l).  b [B][n_m]
        (or one [n_m] for the whole batch) in the powerful basis of R_m, any int64; ext: an Ext from the Plan of (m, qs)
        to this one, or None for m = m'; pp_m: the Plan of index m over p alone (k > 0).  cs_shared: one ciphertext
        ([ncs][1][n][T]) for all B items."""
        _, cs, ncs, Bc = self._cs(cs)
        B = Bc if B is None else int(B)
        n_m = self.n if ext is None else ext.lo.n
        b, stride = self._public(b, n_m, B, stride)
        L, xh, pph = lib(), (None if ext is None else ext._h), (None if pp_m is None else pp_m._h)
        lo = C.c_int64(0)
        args = (int(cs_shared), int(cs_crt), self._enc(enc), int(k), int(l), int(p))
        out = self._run_staged(
            lambda st, i, o, w, nb: L.lolhip_add_public_batch(self._h, xh, pph, st, i[1], stride, i[0], ncs, *args, o,
                                                               C.byref(lo), w, nb),
            stream, (cs, b), B, lambda: L.lolhip_public_work_len(self._h, xh, B), lambda: (ncs, B, self.n, self.T))
        return out, "LSD", int(lo.value)

    def mulPublic(self, a, cs, p, ext=None, cs_shared=False, stride=None, B=None, out=None, stream=None):
        """mulPublic a (SymmSHE.hs:405-411): every c_i times embed (reduce (decode' a)), cs and the result in the CRT
        basis; enc, k and l do not change.  a [B][n_m] (or one [n_m]), any int64, powerful basis of R_m; stride: the
        item stride of a (e.g. L n for KHPRF.eval's [B][L][n]); out may be cs unless cs is shared and B > 1."""
        _, cs, ncs, Bc = self._cs(cs)
        B = Bc if B is None else int(B)
        n_m = self.n if ext is None else ext.lo.n
        a, stride = self._public(a, n_m, B, stride)
        L, xh = lib(), (None if ext is None else ext._h)
        return self._run_staged(
            lambda st, i, o, w, b: L.lolhip_mul_public_batch(self._h, xh, st, i[1], stride, int(p), i[0], ncs,
                                                              int(cs_shared), o, w, b),
            stream, (cs, a), B, lambda: L.lolhip_public_work_len(self._h, xh, B), lambda: (ncs, B, self.n, self.T), out=out)

    def modSwitchPT(self, cs, p, p2, enc="LSD", l=1, stream=None):
        """modSwitchPT from p to p2 | p (SymmSHE.hs:255-261): toMSD, then l' = decode'_p(l) mod p2 -> (cs, "MSD", l')"""
        if int(p) % int(p2):
            raise ValueError("p2 must divide p")
        cs, _, l = self.toMSD(cs, p, enc, l, stream=stream)
        return cs, "MSD", self._decode(l, p) % int(p2)

    def modSwitch(self, to, cs, p, enc="LSD", l=1, cs_crt=False, out_crt=False, stream=None):
        """modSwitch (SymmSHE.hs:236-246) from this plan's moduli to those of `to`, a Plan of the same index whose moduli
        are a suffix of these (up to 5 dropped), of which these are a suffix (up to 5 added), or the same (toMSD):
        lolhip_modswitch_batch, one pass for the encoding scale and the whole rescale.  cs [ncs][B][n][T] in the powerful
        basis (or the CRT basis with cs_crt) -> (out [ncs][B][n][T'] in the basis out_crt asks for, "MSD", l')."""
        _, cs, ncs, B = self._cs(cs)
        L, lo = lib(), C.c_int64(0)
        args = (ncs, int(cs_crt), self._enc(enc), int(l), int(p))
        out = self._run_staged(
            lambda st, i, o, w, b: L.lolhip_modswitch_batch(self._h, to._h, st, i[0], *args, o, int(out_crt),
                                                             C.byref(lo), w, b),
            stream, (cs,), B, lambda: L.lolhip_modswitch_work_len(self._h, to._h, ncs, B), lambda: (ncs, B, to.n, to.T))
        return out, "MSD", int(lo.value)

    def ctAffineMul(self, a, alpha, b=None, beta=1, va=None, vb=None, npairs=1, out=None, stream=None):
        """The ciphertext product with both affine pre-steps folded in (lolhip_ct_affine_mul_batch), CRT basis: for every
        pair j, (g A0 B0, g (A0 B1 + A1 B0), g A1 B1) with A0 = alpha a_0 + va_j, A1 = alpha a_1, B0 = beta b_0 + vb_j,
        B1 = beta b_1.  a, b [2][B][n][T] (b None: b = a, read once); alpha, beta: an int or one int per modulus; va, vb
        [npairs][n][T] or None -> [npairs][3][B][n][T].  With npairs = 1, out may be a or b."""
        import torch
        host, a, na, B = self._cs(a)
        if b is not None:
            _, b, nb, Bb = self._cs(b)
            if Bb != B or nb != 2:
                raise ValueError("b is not a linear ciphertext of a's batch")
        if na != 2:
            raise ValueError("a is not a linear ciphertext [2][B][n][T]")
        al, be, L, npairs = self._per_mod(alpha), self._per_mod(beta), lib(), int(npairs)
        _check(L.lolhip_ct_affine_mul_batch(self._h, None, None, al, None, None, be, None, npairs, None, 0))
        if host:
            _, (a, b, va, vb) = self._stage(a, b, va, vb)
        for v in (va, vb):
            if v is not None and v.numel() != npairs * self.n * self.T:
                raise ValueError("va / vb are not [npairs][n][T]")
        if out is None:
            out = torch.empty((npairs, 3, B, self.n, self.T), dtype=torch.int64, device=a.device)
        opt = lambda t: None if t is None else _devptr(t)
        _check(L.lolhip_ct_affine_mul_batch(self._h, _stream(stream), _devptr(a), al, opt(va), _devptr(a if b is None else b),
                                            be, opt(vb), npairs, _devptr(out), B))
        return self._unstage(host, out)

    def absorbGFactors(self, cs, k, pp, stream=None):
        """absorbGFactors (SymmSHE.hs:464-473) of a CRT-basis ciphertext: every c_i times decode'(divG^k 1), divG over
        pp (the Plan of this index over p alone) -> (cs, 0)"""
        if int(k) == 0:
            return cs, 0
        d = np.zeros((1, pp.n, 1), dtype=np.int64)
        d[0, 0, 0] = 1
        for _ in range(int(k)):
            d = pp.divGPow(d)
            if d is None:
                raise LolHipError(ERR_NOT_DIVISIBLE, "absorbGFactors: divG mod p")
        if not isinstance(cs, np.ndarray) and not isinstance(cs, (list, tuple)):
            import torch
            d = torch.from_numpy(d).to(cs.device)
        return self.mulPublic(d.reshape(-1) if isinstance(d, np.ndarray) else d.reshape(-1), cs, pp.qs[0], stride=0,
                              stream=stream), 0


def mulC(a, b, stream=None):
    """a * b elementwise over complex128 (mulC, types.h:146-152: each product and each sum rounded on its own): with
    crtC / crtInvC the reference's product for moduli without a CRT basis (UCyc CRTExt).  numpy in -> numpy out; a torch
    CUDA tensor a is overwritten.  b may be a."""
    import torch
    host = isinstance(a, np.ndarray)
    ta = torch.from_numpy(np.ascontiguousarray(a, dtype=np.complex128)).cuda() if host else a
    tb = ta if b is a else (torch.from_numpy(np.ascontiguousarray(b, dtype=np.complex128)).cuda() if isinstance(b, np.ndarray) else b)
    for t in (ta, tb):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.complex128):
            raise TypeError("expected contiguous complex128 arrays or CUDA tensors")
    if ta.numel() != tb.numel():
        raise ValueError("operand sizes differ")
    _check(lib().lolhip_mulc_batch(_stream(stream), ta.data_ptr(), tb.data_ptr(), ta.numel()), "mulc")
    return ta.cpu().numpy() if host else ta


def chacha20_block(key, counter, nonce):
    """The ChaCha20 block function the samplers run (RFC 8439 §2.3), on the host: 16 uint32 words."""
    kb = bytes(key)
    if len(kb) != 32:
        raise ValueError("key must be 32 bytes")
    nn = (C.c_uint32 * 3)(*[int(x) & 0xFFFFFFFF for x in nonce])
    out = (C.c_uint32 * 16)()
    lib().lolhip_chacha20_block(kb, int(counter) & 0xFFFFFFFF, nn, out)
    return np.array(list(out), dtype=np.uint32)


class Ext:
    """Index tables and kernels for a ring extension m | m' (Tensor.hs:390-509, Extension.hs:54-129)."""

    def __init__(self, lo: Plan, hi: Plan):
        self.lo, self.hi = lo, hi
        h = C.c_void_p()
        _check(lib().lolhip_ext_create(lo._h, hi._h, C.byref(h)), "ext_create")
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.lolhip_ext_destroy(h)

    def table(self, which):
        L = lib()
        cnt = L.lolhip_ext_table(self._h, which, None, 0)
        out = np.zeros(cnt, dtype=np.int32)
        if cnt:
            L.lolhip_ext_table(self._h, which, out.ctypes.data_as(_i32p), cnt)
        return out

    def powBasisPow(self):
        """powBasisPow (CPP/Extension.hs:131-141): the n'/n powerful-basis indices at which the relative powerful basis
        elements of O_m'/O_m are unit vectors; sum_i embedPow(coeffs_i x) b_i = x."""
        return self.table(6)

    def _run(self, op, name, x, to_hi, out, stream):
        src, dst = (self.lo, self.hi) if to_hi else (self.hi, self.lo)
        if isinstance(x, np.ndarray):
            x, xp = _np(x)
            B = src._batch(x)
            res = np.zeros((B, dst.n, dst.T), dtype=np.int64)
            _check(lib().lolhip_ext_host(self._h, op, res.ctypes.data_as(_i64p), xp, B))
            return res
        B = src._batch_t(x)
        if out is None:
            import torch
            out = torch.empty((B, dst.n, dst.T), dtype=torch.int64, device=x.device)
        _check(getattr(lib(), f"lolhip_{name}_batch")(self._h, _stream(stream), _devptr(out), _devptr(x), B))
        return out

    def coeffs(self, x, out=None, stream=None):
        """[n'/n][B][n][T] coefficient vectors over the relative powerful/decoding basis (Tensor.hs:174)."""
        rel = self.hi.n // self.lo.n
        if isinstance(x, np.ndarray):
            x, xp = _np(x)
            B = self.hi._batch(x)
            res = np.zeros((rel, B, self.lo.n, self.lo.T), dtype=np.int64)
            _check(lib().lolhip_ext_host(self._h, EXT_COEFFS, res.ctypes.data_as(_i64p), xp, B))
            return res
        B = self.hi._batch_t(x)
        if out is None:
            import torch
            out = torch.empty((rel, B, self.lo.n, self.lo.T), dtype=torch.int64, device=x.device)
        _check(lib().lolhip_coeffs_batch(self._h, _stream(stream), _devptr(out), _devptr(x), B))
        return out

    def evalLin(self, es: "Ext", r_dec, ys_crt, stream=None):
        """sum_i ys_i * embed(coeffsDec_i r)  (Linear.hs:75-79): self = E in R, es = E in S;
        r_dec [B][n_R][T] decoding basis, ys_crt [n_R/n_E][n_S][T] CRT basis -> [B][n_S][T] CRT basis."""
        import torch
        host, (r_dec, ys_crt) = Plan._stage(r_dec, ys_crt)
        B, rel = self.hi._batch_t(r_dec), self.hi.n // self.lo.n
        S = es.hi
        work = torch.empty((rel * B * (self.lo.n + S.n) * S.T,), dtype=torch.int64, device=r_dec.device)
        out = torch.empty((B, S.n, S.T), dtype=torch.int64, device=r_dec.device)
        _check(lib().lolhip_evallin_batch(self._h, es._h, _stream(stream), _devptr(r_dec), _devptr(ys_crt),
                                          _devptr(out), _devptr(work), B))
        return Plan._unstage(host, out)

    def tunnel(self, es: "Ext", c0_dec, c1_pow, ys_crt, hints, base, stream=None):
        """SymmSHE `tunnel` after toMSD . absorbGFactors (SymmSHE.hs:549-570): self = E' in R', es = E' in S';
        [c0 (decoding basis), c1 (powerful basis)] over R' -> [2][B][n_S][T] CRT-basis linear ciphertext over S'.
        hints [n_R/n_E][L][2][n_S][T]."""
        import torch
        host, (c0_dec, c1_pow, ys_crt, hints) = Plan._stage(c0_dec, c1_pow, ys_crt, hints)
        B, S = self.hi._batch_t(c0_dec), es.hi
        wl = lib().lolhip_tunnel_work_len(self._h, es._h, int(base), B)
        _check(min(wl, 0))
        work = torch.empty((max(wl, 1),), dtype=torch.int64, device=c0_dec.device)
        out = torch.empty((2, B, S.n, S.T), dtype=torch.int64, device=c0_dec.device)
        _check(lib().lolhip_tunnel_batch(self._h, es._h, _stream(stream), _devptr(c0_dec), _devptr(c1_pow), _devptr(ys_crt),
                                         _devptr(hints), int(base), _devptr(out), _devptr(work), B))
        return Plan._unstage(host, out)

    def tunnelHint(self, es: "Ext", ys_crt, s_in_crt, s_out_crt, svar, base, key=None, ctr=0, stream=None):
        """tunnelHint f skout skin (SymmSHE.hs:531-545): self = E' in R', es = E' in S'; ys_crt [rel][n_S][T] the
        linearDec table of f'q (what tunnel takes), s_in_crt [n_R][T] and s_out_crt [n_S][T] the keys in the CRT bases
        -> hints [rel][L][2][n_S][T] for tunnel.  Uses stream items ctr .. ctr + rel L - 1."""
        import torch
        L = lib()
        kb = Plan._key(key)
        R, S = self.hi, es.hi
        rel = R.n // self.lo.n
        shapes = [(ys_crt, rel * S.n * S.T), (s_in_crt, R.n * R.T), (s_out_crt, S.n * S.T)]
        if any((a.size if isinstance(a, np.ndarray) else a.numel()) != want for a, want in shapes):
            raise LolHipError(ERR_INVALID, "tunnelHint: ys_crt, s_in_crt or s_out_crt is not of the plans of the extensions")
        wl = L.lolhip_tunnel_hint_work_len(self._h, es._h, int(base))
        _check(min(wl, 0))
        host, (ys_crt, s_in_crt, s_out_crt) = Plan._stage(ys_crt, s_in_crt, s_out_crt)
        dev = ys_crt.device
        work = torch.empty((max(wl, 1),), dtype=torch.int64, device=dev)
        out = torch.empty((rel, S.decomposeLen(base), 2, S.n, S.T), dtype=torch.int64, device=dev)
        _check(L.lolhip_tunnel_hint_batch(self._h, es._h, _stream(stream), _devptr(ys_crt), _devptr(s_in_crt),
                                          _devptr(s_out_crt), float(svar), int(base), kb, int(ctr), _devptr(out),
                                          _devptr(work)))
        return Plan._unstage(host, out)

    def twacePowDec(self, x, out=None, stream=None): return self._run(EXT_TWACE_POWDEC, "twace_powdec", x, False, out, stream)
    def twaceCRT(self, x, out=None, stream=None): return self._run(EXT_TWACE_CRT, "twace_crt", x, False, out, stream)
    def embedPow(self, x, out=None, stream=None): return self._run(EXT_EMBED_POW, "embed_pow", x, True, out, stream)
    def embedDec(self, x, out=None, stream=None): return self._run(EXT_EMBED_DEC, "embed_dec", x, True, out, stream)
    def embedCRT(self, x, out=None, stream=None): return self._run(EXT_EMBED_CRT, "embed_crt", x, True, out, stream)


class TunnelChain:
    """tunnelH (HomomPRF.hs:427-431): roundCTUp, the tunnel hops and the roundCTDowns as one call
    (lolhip_tunnel_chain_batch).  exts_er[i] / exts_es[i]: the Exts E'_i in R'_i / E'_i in S'_i of hop i, all over one
    moduli list (the up list); ys[i] [rel_i][n_S][T] and hints[i] [rel_i][L][2][n_S][T]: CUDA tensors as Ext.tunnel
    takes them (kept alive here); p_in / p_out: Plans of the first R' / last S' index over a suffix of the up list."""

    def __init__(self, exts_er, exts_es, ys, hints, base, p_in: Plan, p_out: Plan):
        self.exts_er, self.exts_es, self.ys, self.hint_slabs = list(exts_er), list(exts_es), list(ys), list(hints)
        self.base, self.p_in, self.p_out = int(base), p_in, p_out
        n = len(self.exts_er)
        if not (len(self.exts_es) == len(self.ys) == len(self.hint_slabs) == n):
            raise ValueError("one ext pair, one ys table and one hint slab per hop")
        arr = lambda vals: (C.c_void_p * max(n, 1))(*vals)
        h = C.c_void_p()
        _check(lib().lolhip_tunnel_chain_create(n, arr([x._h for x in self.exts_er]), arr([x._h for x in self.exts_es]),
                                                arr([_devptr(y) for y in self.ys]), arr([_devptr(x) for x in self.hint_slabs]),
                                                self.base, p_in._h, p_out._h, C.byref(h)), "tunnel_chain_create")
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.lolhip_tunnel_chain_destroy(h)

    def workLen(self, B):
        w = lib().lolhip_tunnel_chain_work_len(self._h, int(B))
        _check(min(w, 0))
        return w

    def __call__(self, cs, p, enc="LSD", l=1, cs_crt=False, out_crt=False, stream=None):
        """cs [2][B][n_R'][T_in], a linear ciphertext with k = 0 (Plan.absorbGFactors first otherwise), powerful basis or
        CRT basis (cs_crt) -> (out [2][B][n_S'][T_out], "MSD", l')."""
        _, cs, ncs, B = self.p_in._cs(cs)
        if ncs != 2:
            raise LolHipError(ERR_INVALID, "tunnelH takes a linear ciphertext")
        L, lo = lib(), C.c_int64(0)
        args = (int(cs_crt), Plan._enc(enc), int(l), int(p))
        out = Plan._run_staged(
            lambda st, i, o, w, b: L.lolhip_tunnel_chain_batch(self._h, st, i[0], *args, o, int(out_crt), C.byref(lo), w, b),
            stream, (cs,), B, lambda: self.workLen(B), lambda: (2, B, self.p_out.n, self.p_out.T))
        return out, "MSD", int(lo.value)

    @staticmethod
    def hints(exts_er, exts_es, exts_f, funcs, s_in_crt, p, svar, base, key=None, ctr=0, stream=None):
        """tunnelHintChain (HomomPRF.hs:400-411) on the device.  Per hop i: a fresh key of S'_i by errorRounded svar
        (genSKWithVar), ys_i = crt (reduce (embed (liftPow f_i))) (extendLin, Linear.hs:113-119) and Ext.tunnelHint.
        exts_er / exts_es as for the chain; exts_f[i]: the Ext from (S_i, up list) to S'_i (None for S = S');
        funcs[i] [rel_i][n_S_i]: the values of the linear function f_i on the relative decoding basis, residues mod p
        in the powerful basis of S_i; s_in_crt [n_R'][T]: the key of R'_0 in the CRT basis.  Stream items: the key of
        hop i is errorRounded's item ctr (domain 2), its hint rows are items ctr .. ctr + rel_i L - 1 of the hint domains
        (3 / 4), and ctr then advances by rel_i L, as include/lolhip.h prescribes.
        Returns (hints, ys, last key [n_S'][T] in the CRT basis, the next free ctr)."""
        import torch
        kb = Plan._key(key)
        s_in = torch.from_numpy(np.ascontiguousarray(s_in_crt, dtype=np.int64)).cuda() if isinstance(s_in_crt, np.ndarray) else s_in_crt
        out_h, out_y = [], []
        for er, es, xf, f in zip(exts_er, exts_es, exts_f, funcs):
            S = es.hi
            qs = torch.tensor(S.qs, dtype=torch.int64, device=s_in.device)
            rel = er.hi.n // er.lo.n
            sk = S.errorRounded(svar, 1, key=kb, ctr=ctr, stream=stream)                      # [1][n_S] decoding basis
            s_out = torch.remainder(sk.reshape(1, S.n, 1), qs).contiguous()
            S.crt(S.l(s_out, stream), stream)
            f = torch.from_numpy(np.ascontiguousarray(f, dtype=np.int64)).to(s_in.device) if isinstance(f, np.ndarray) else f
            f = torch.remainder(f.reshape(rel, -1), int(p))
            f = torch.where(2 * f >= int(p), f - int(p), f)                                     # liftPow: centred
            y = torch.remainder(f.reshape(rel, -1, 1), qs).contiguous()                         # reduce
            y = S.crt(y if xf is None else xf.embedPow(y, stream=stream), stream)
            L = S.decomposeLen(base)
            out_h.append(er.tunnelHint(es, y, s_in.reshape(-1), s_out.reshape(-1), svar, base, key=kb, ctr=ctr,
                                       stream=stream))
            out_y.append(y)
            ctr += rel * L
            s_in = s_out.reshape(S.n, S.T)
        return out_h, out_y, s_in, ctr


    @staticmethod
    def funcs(rings, p, e, host=False, stream=None):
        """The linear functions of tunnelHintChain / ptTunnelFuncs (HomomPRF.hs:400-411, 516-531) for the plaintext rings
        rings = [r_0, ..., r_H] (indices): per hop h, with e_h = gcd(r_h, r_(h+1)) and dim_h = phi(r_h) / phi(e_h), the
        first dim_h elements of crtSet(e_h, r_(h+1), p, e) as [dim_h][n_S_h] residues mod p^e, powerful basis: the values
        of f_h on the relative decoding basis, the `funcs` of TunnelChain.hints and PTTunnel.  CUDA tensors, or numpy
        with host=True (crtSet's host path).  ValueError when a hop's CRT set has fewer than dim_h elements."""
        import math
        out = []
        for r, s_ in zip(rings[:-1], rings[1:]):
            eh = math.gcd(int(r), int(s_))
            dim = _totient(factor_pps(int(r))) // _totient(factor_pps(eh))
            cs = crtSet(eh, int(s_), p, e, host=host, stream=stream)
            if cs.shape[0] < dim:
                raise ValueError(f"the CRT set of O_{s_}/O_{eh} mod {p} has {cs.shape[0]} elements, the hop from {r} needs {dim}")
            out.append(cs[:dim].copy() if host else cs[:dim].contiguous())
        return out


class PTTunnel:
    """ptTunnel (HomomPRF.hs:510-531): evalLin f_h hop by hop on plaintexts over Z_(p^e) as one call
    (lolhip_pt_tunnel_batch).  exts_er[h] / exts_es[h]: the Exts E_h in R_h / E_h in S_h over ONE NTT prime Q_h per hop
    that exceeds PTTunnel.modulus (certified at creation); funcs[h] [rel_h][n_S_h]: the values of f_h on the relative
    decoding basis, residues mod p^e in the powerful basis (TunnelChain.funcs; numpy or CUDA tensors)."""

    def __init__(self, exts_er, exts_es, funcs, p, e):
        self.exts_er, self.exts_es, self.p, self.e = list(exts_er), list(exts_es), int(p), int(e)
        n = len(self.exts_er)
        if not (len(self.exts_es) == len(funcs) == n):
            raise ValueError("one ext pair and one function table per hop")
        fs = []
        for x, f in zip(self.exts_er, funcs):
            f = np.ascontiguousarray(f if isinstance(f, np.ndarray) else f.cpu().numpy(), dtype=np.int64)
            if f.size != (x.hi.n // x.lo.n) * self.exts_es[len(fs)].hi.n:
                raise ValueError("funcs[h] must be [n_R/n_E][n_S]")
            fs.append(f)
        arr = lambda vals: (C.c_void_p * max(n, 1))(*vals)
        fp = (_i64p * max(n, 1))(*[f.ctypes.data_as(_i64p) for f in fs])
        h = C.c_void_p()
        _check(lib().lolhip_pt_tunnel_create(n, arr([x._h for x in self.exts_er]), arr([x._h for x in self.exts_es]), fp,
                                             self.p, self.e, C.byref(h)), "pt_tunnel_create")
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.lolhip_pt_tunnel_destroy(h)

    @staticmethod
    def modulus(pps_r, pps_s, rel, first_hop, p, e):
        """The exactness bound of one hop (include/lolhip.h): the hop's prime Q must exceed the returned value."""
        (_, a, na), (_, b, nb) = _pps(pps_r), _pps(pps_s)
        v = lib().lolhip_pt_tunnel_modulus(a, na, b, nb, int(rel), int(bool(first_hop)), int(p), int(e))
        _check(min(v, 0), "pt_tunnel_modulus")
        return int(v)

    @classmethod
    def for_rings(cls, rings, p, e, funcs=None, host_only=False):
        """The tunnel over the plaintext rings [r_0, ..., r_H] with the functions of TunnelChain.funcs (or `funcs`): per
        hop the plans of E_h = gcd, R_h and S_h over the smallest admissible prime Q_h = 1 mod r_(h+1)."""
        import math
        if funcs is None:
            funcs = TunnelChain.funcs(rings, p, e, host=host_only)
        er, es = [], []
        for h, (r, s_) in enumerate(zip(rings[:-1], rings[1:])):
            eh = math.gcd(int(r), int(s_))
            rel = _totient(factor_pps(int(r))) // _totient(factor_pps(eh))
            Q = good_q(int(s_), cls.modulus(int(r), int(s_), rel, h == 0, p, e))
            E, R, S = (Plan.for_index(m, [Q], host_only=host_only) for m in (eh, int(r), int(s_)))
            er.append(Ext(E, R))
            es.append(Ext(E, S))
        return cls(er, es, funcs, p, e)

    def workLen(self, B):
        w = lib().lolhip_pt_tunnel_work_len(self._h, int(B))
        _check(min(w, 0))
        return w

    def __call__(self, x_dec, stream=None):
        """x_dec [B][n_R0]: plaintexts mod p^e in the decoding basis of R_0 (numpy or a CUDA tensor) -> [B][n_S] residues
        in [0, p^e), powerful basis of the last ring."""
        import torch
        L = lib()
        _check(L.lolhip_pt_tunnel_batch(self._h, None, None, None, None, 0))          # the host statuses first
        host = isinstance(x_dec, np.ndarray)
        x = torch.from_numpy(np.ascontiguousarray(x_dec, dtype=np.int64)).cuda() if host else x_dec
        nR, nS = self.exts_er[0].hi.n, self.exts_es[-1].hi.n
        if x.numel() % nR:
            raise ValueError("x_dec is not a whole number of plaintexts of R_0")
        B = x.numel() // nR
        work = torch.empty((max(self.workLen(B), 2),), dtype=torch.int64, device=x.device)
        out = torch.empty((B, nS), dtype=torch.int64, device=x.device)
        _check(L.lolhip_pt_tunnel_batch(self._h, _stream(stream), _devptr(x), _devptr(out), _devptr(work), B))
        return out.cpu().numpy() if host else out


class RingMul:
    """The exact ring product a * b in R_q for moduli without a CRT basis (lolhip_ringmul_batch): q = 2^e, p^e, odd
    composites, tuples of them.  plan_q: any Plan over the moduli; plan_Q: a Plan of the same index over K <= 3 distinct
    NTT primes whose product exceeds 2 C_m floor(q/2)^2 (certified at creation), or None for the primes of
    RingMul.moduli.  Operands and results [B][n][T], powerful basis, numpy or CUDA tensors; operands may be any int64
    (taken mod q_t), results lie in [0, q_t)."""

    def __init__(self, plan_q, plan_Q=None):
        if plan_Q is None:
            plan_Q = Plan(plan_q.pps, self.moduli(plan_q.pps, plan_q.qs), host_only=plan_q.host_only)
        self.plan_q, self.plan_Q = plan_q, plan_Q
        self.n, self.T, self.K = plan_q.n, plan_q.T, plan_Q.T
        h = C.c_void_p()
        _check(lib().lolhip_ringmul_create(plan_q._h, plan_Q._h, C.byref(h)), "ringmul_create")
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.lolhip_ringmul_destroy(h)

    @staticmethod
    def moduli(pps, qs):
        """The default NTT primes for index `pps` (a prime-power list or m) and moduli qs: the fewest K <= 3 consecutive
        primes = 1 mod m above the K-th root of 2 C_m floor(max q / 2)^2 (the rule of include/lolhip.h)."""
        _, a, na = _pps(pps)
        qa = (C.c_int64 * max(1, len(qs)))(*[int(q) for q in qs])
        Qs = (C.c_int64 * 3)()
        K = lib().lolhip_ringmul_moduli(a, na, qa, len(qs), Qs)
        _check(min(K, 0), "ringmul_moduli")
        return [int(Qs[i]) for i in range(K)]

    def workLen(self, B):
        w = lib().lolhip_ringmul_work_len(self._h, int(B))
        _check(min(w, 0))
        return w

    def _batch(self, a):
        per, size = self.n * self.T, self._size(a)
        if size % per:
            raise ValueError(f"not a whole number of [n={self.n}, T={self.T}] ring elements")
        return size // per

    @staticmethod
    def _size(x):
        return x.size if isinstance(x, np.ndarray) else x.numel()

    def __call__(self, a, b, out=None, stream=None):
        """out = a * b; out may be a or b (CUDA tensors), and a may be b."""
        L, B = lib(), self._batch(a)
        if self._batch(b) != B:
            raise ValueError("a and b hold different batches")
        same = b is a
        call = lambda s, p, o, w, n: L.lolhip_ringmul_batch(self._h, s, o, p[0], p[0] if same else p[1], w, n)
        return Plan._run_staged(call, stream, [a] if same else [a, b], B, lambda: self.workLen(B),
                                lambda: (B, self.n, self.T), out=out)

    def prepare(self, b, stream=None):
        """bhat [Bb T][n][K]: the CRT over plan_Q of the lifted b [Bb][n][T], for mulPrepared."""
        L, Bb = lib(), self._batch(b)
        call = lambda s, p, o, w, n: L.lolhip_ringmul_prepare(self._h, s, o, p[0], w, n)
        return Plan._run_staged(call, stream, [b], Bb, lambda: 0, lambda: (Bb * self.T, self.n, self.K))

    def mulPrepared(self, a, bhat, out=None, stream=None):
        """out = a * b for bhat = prepare(b) of one element (against every item of a) or of as many as a holds."""
        L, B = lib(), self._batch(a)
        per = self.T * self.n * self.K
        size = self._size(bhat)
        if size % per:
            raise ValueError("bhat is not a whole number of prepared elements")
        Bb = size // per
        call = lambda s, p, o, w, n: L.lolhip_ringmul_prepared_batch(self._h, s, o, p[0], p[1], Bb, w, n)
        return Plan._run_staged(call, stream, [a, bhat], B, lambda: self.workLen(B), lambda: (B, self.n, self.T), out=out)


class PTRound:
    """ptRound (HomomPRF.hs:215-270): homomorphic rounding from plaintext modulus p = 2^e to 2 as one call
    (lolhip_ptround_batch).  plans[i], i < e: the Plan of index m' over Z_i, each list the one before without its first
    modulus; up_plans[i], i < e - 1: the Plan over U_i = one more modulus in front of Z_i; hints[i] [L_i][2][n'][T(U_i)]:
    ksQuadCircHint of the key over U_i as CUDA tensors (kept alive here; PTRound.hints makes them); pp_m: the Plan of
    index m over p alone (made here when None); exts: (Ext from (m, Z_0) to plans[0], Ext from (m, Z_1) to plans[1]), or
    None for m = m'."""

    def __init__(self, plans, up_plans, hints, base, p, pp_m=None, exts=None):
        self.plans, self.up_plans, self.hint_slabs = list(plans), list(up_plans), list(hints)
        self.base, self.p, self.exts = int(base), int(p), (None if exts is None else tuple(exts))
        e = len(self.plans)
        if e < 1 or len(self.up_plans) != e - 1 or len(self.hint_slabs) != e - 1:
            raise ValueError("e plans, e - 1 up plans and e - 1 hints")
        if pp_m is None and e > 1:
            lo = self.plans[0] if self.exts is None else self.exts[0].lo
            pp_m = Plan(lo.pps, [self.p])
        self.pp_m = pp_m
        arr = lambda vals: (C.c_void_p * max(len(vals), 1))(*vals)
        xs = (None, None) if self.exts is None else tuple(None if x is None else x._h for x in self.exts)
        h = C.c_void_p()
        _check(lib().lolhip_ptround_create(e, self.p, arr([q._h for q in self.plans]), arr([q._h for q in self.up_plans]),
                                           arr([_devptr(x) for x in self.hint_slabs]), self.base,
                                           None if pp_m is None else pp_m._h, xs[0], xs[1] if e > 1 else None, C.byref(h)),
               "ptround_create")
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.lolhip_ptround_destroy(h)

    def workLen(self, B):
        w = lib().lolhip_ptround_work_len(self._h, int(B))
        _check(min(w, 0))
        return w

    def __call__(self, cs, enc="MSD", k=0, l=1, cs_crt=False, out_crt=False, stream=None):
        """cs [2][B][n'][T(Z_0)]: CT enc k l over plaintext modulus p, powerful basis or CRT basis (cs_crt) ->
        (out [2][B][n'][T(Z_{e-1})], "MSD", k_out, l_out) over plaintext modulus 2; for e = 1 the input itself, its
        encoding, k and l unchanged."""
        _, cs, ncs, B = self.plans[0]._cs(cs)
        if ncs != 2:
            raise LolHipError(ERR_INVALID, "ptRound takes a linear ciphertext")
        L, ko, lo, last = lib(), C.c_int64(0), C.c_int64(0), self.plans[-1]
        args = (int(cs_crt), Plan._enc(enc), int(k), int(l))
        out = Plan._run_staged(
            lambda st, i, o, w, b: L.lolhip_ptround_batch(self._h, st, i[0], *args, o, int(out_crt), C.byref(ko), C.byref(lo),
                                                           w, b),
            stream, (cs,), B, lambda: self.workLen(B), lambda: (2, B, last.n, last.T))
        return out, ("MSD" if len(self.plans) > 1 else ("LSD", "MSD")[Plan._enc(enc)]), int(ko.value), int(lo.value)

    @staticmethod
    def hints(up_plans, s_crts, svar, base, key=None, ctr=0, stream=None):
        """roundHints (HomomPRF.hs:255-258) on the device: one Plan.ksQuadCircHint per level, over U_i.  s_crts[i]
        [n'][T(U_i)]: the key reduced into U_i's moduli, CRT basis.  Stream items: level i draws its L_i =
        up_plans[i].decomposeLen(base) LWE samples at items ctr_i .. ctr_i + L_i - 1 of the hint domains, ctr_0 = ctr and
        ctr_(i+1) = ctr_i + L_i, so two levels never share a stream block under one key.
        Returns (hints, the next free ctr)."""
        out = []
        for U, s in zip(up_plans, s_crts):
            out.append(U.ksQuadCircHint(s, svar, base, key=key, ctr=ctr, stream=stream))
            ctr += U.decomposeLen(base)
        return out, ctr


# ---- key-homomorphic ring PRF (lol-apps KeyHomomorphicPRF.hs) -------------------------------
# Trees are preorder lists of leaf counts: 1 for a leaf, a node of c > 1 leaves followed by its left, then its right
# subtree (I 3 L (I 2 L L) = [3, 1, 2, 1, 1]).

def left_spine_tree(k):
    """leftSpineTree k (KeyHomomorphicPRF.hs): I k (leftSpineTree (k-1)) L"""
    return [1] if k == 1 else [k] + left_spine_tree(k - 1) + [1]


def right_spine_tree(k):
    """rightSpineTree k: I k L (rightSpineTree (k-1))"""
    return [1] if k == 1 else [k, 1] + right_spine_tree(k - 1)


def balanced_tree(k):
    """balancedTree k: the left subtree takes min(2^floor(log2 k), k - 2^floor(log2 k) / 2) leaves"""
    if k == 1:
        return [1]
    full = 1 << (k.bit_length() - 1)
    lsize = min(full, k - full // 2)
    return [k] + balanced_tree(lsize) + balanced_tree(k - lsize)


def gray_code(k):
    """grayCode k: the (k-1)-bit code, then its reverse with bit k-1 set"""
    if k == 1:
        return [0, 1]
    g = gray_code(k - 1)
    return g + [x + (1 << (k - 1)) for x in reversed(g)]


class KHPRF:
    """A family of the key-homomorphic ring PRF of [BP14] over a one-modulus plan (lolhip_khprf_create): a full binary
    tree (preorder leaf counts) and a0, a1 [L][n] in the CRT basis, L = plan.decomposeLen(base).  On a device plan a0,
    a1 and their crt'd gadget decompositions go to HBM once; a host-only plan answers workLen only."""

    def __init__(self, plan: Plan, base, tree, a0, a1):
        self.plan, self.base = plan, int(base)
        self.tree = [int(c) for c in tree]
        self.L = plan.decomposeLen(base) if plan.T == 1 else 0
        a0 = np.ascontiguousarray(np.asarray(a0, dtype=np.int64).reshape(-1))
        a1 = np.ascontiguousarray(np.asarray(a1, dtype=np.int64).reshape(-1))
        if a0.size != self.L * plan.n or a1.size != self.L * plan.n:
            raise ValueError("a0 and a1 must be [L][n]")
        tr = (C.c_int32 * max(1, len(self.tree)))(*self.tree)
        h = C.c_void_p()
        _check(lib().lolhip_khprf_create(plan._h, self.base, tr, len(self.tree), a0.ctypes.data_as(_i64p),
                                         a1.ctypes.data_as(_i64p), C.byref(h)), f"khprf_create(tree={self.tree})")
        self._h = h
        self.k = self.tree[0]
        self.plan_Q = None

    @classmethod
    def lifted(cls, plan_q: Plan, plan_Q: Plan, base, tree, a0_pow, a1_pow):
        """The same PRF over q = 2^k, which has no CRT basis (lolhip_khprf_create_lifted): plan_q mod q, plan_Q of the
        same index over an NTT-friendly prime Q in which every node product is exact (certified here), a0_pow, a1_pow
        [L][n] in the powerful basis.  eval() then returns A_T(x) in the powerful basis mod q, and a key s passed to
        __call__ is in the powerful basis of R_q."""
        self = cls.__new__(cls)
        self.plan, self.plan_Q, self.base = plan_q, plan_Q, int(base)
        self.tree = [int(c) for c in tree]
        self.L = plan_q.decomposeLen(base) if plan_q.T == 1 else 0
        a0 = np.ascontiguousarray(np.asarray(a0_pow, dtype=np.int64).reshape(-1))
        a1 = np.ascontiguousarray(np.asarray(a1_pow, dtype=np.int64).reshape(-1))
        if a0.size != self.L * plan_q.n or a1.size != self.L * plan_q.n:
            raise ValueError("a0 and a1 must be [L][n]")
        tr = (C.c_int32 * max(1, len(self.tree)))(*self.tree)
        h = C.c_void_p()
        _check(lib().lolhip_khprf_create_lifted(plan_q._h, plan_Q._h, self.base, tr, len(self.tree),
                                                a0.ctypes.data_as(_i64p), a1.ctypes.data_as(_i64p), C.byref(h)),
               f"khprf_create_lifted(tree={self.tree})")
        self._h = h
        self.k = self.tree[0]
        return self

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.lolhip_khprf_destroy(h)

    def _key_crt(self, s, nkeys, stream=None):
        """the lifted family's keys: powerful basis of R_q -> centred lift mod Q -> crt on plan_Q.  A CUDA key stays on
        the device (torch ops ordered on the call's stream); a numpy key is lifted before its upload."""
        import torch
        q, Q = self.plan.qs[0], self.plan_Q.qs[0]
        ctx = torch.cuda.stream(torch.cuda.ExternalStream(int(stream))) if stream else contextlib.nullcontext()
        with ctx:
            if isinstance(s, np.ndarray):
                r = np.asarray(s, dtype=np.int64).reshape(nkeys, self.plan.n) & (q - 1)
                d = torch.from_numpy(np.ascontiguousarray(np.where(2 * r < q, r, r - q + Q))).cuda()
            else:
                r = s.to(torch.int64).reshape(nkeys, self.plan.n) & (q - 1)
                d = torch.where(2 * r < q, r, r - q + Q).contiguous()
        self.plan_Q.crt(d.view(nkeys, self.plan.n, 1), stream)
        return d

    def workLen(self, x0, B):
        w = lib().lolhip_khprf_work_len(self._h, int(x0), int(B))
        _check(min(w, 0))
        return w

    def eval(self, x0, B, stream=None):
        """A_T(x) for x = x0 .. x0 + B - 1: a CUDA tensor [B][L][n] in the CRT basis (lolhip_khprf_eval_batch); the
        lifted family: in the powerful basis, residues in [0, q)."""
        import torch
        L = lib()
        _check(L.lolhip_khprf_eval_batch(self._h, None, int(x0), 0, None, None))      # the host statuses first
        if int(x0) + int(B) > (1 << self.k) or int(B) < 0:
            _check(ERR_INVALID, "x0 + B > 2^k")
        work = torch.empty((max(self.workLen(x0, B), 1),), dtype=torch.int64, device="cuda")
        out = torch.empty((int(B), self.L, self.plan.n), dtype=torch.int64, device="cuda")
        _check(L.lolhip_khprf_eval_batch(self._h, _stream(stream), int(x0), int(B), _devptr(out), _devptr(work)))
        return out

    def __call__(self, s, p, x0, B, stream=None):
        """ringPRF s x for x = x0 .. x0 + B - 1 (lolhip_khprf_batch): s [n] or [nkeys][n] in the CRT basis (numpy or a
        CUDA tensor; the lifted family: in the powerful basis of R_q) -> [nkeys][B][L][n] int64 in [0, p), decoding
        basis of R_p ([B][L][n] for a single key s [n])."""
        import torch
        L = lib()
        single = len(s.shape) == 1
        nkeys = 1 if single else int(s.shape[0])
        _check(L.lolhip_khprf_batch(self._h, None, None, nkeys, int(p), int(x0), 0, None, None))
        if int(x0) + int(B) > (1 << self.k) or int(B) < 0:
            _check(ERR_INVALID, "x0 + B > 2^k")
        if self.plan_Q is not None:
            s = self._key_crt(s, nkeys, stream)
        elif isinstance(s, np.ndarray):
            s = torch.from_numpy(np.ascontiguousarray(s, dtype=np.int64)).cuda()
        s = s.reshape(nkeys, self.plan.n).contiguous()
        work = torch.empty((max(self.workLen(x0, B), 1),), dtype=torch.int64, device=s.device)
        out = torch.empty((nkeys, int(B), self.L, self.plan.n), dtype=torch.int64, device=s.device)
        _check(L.lolhip_khprf_batch(self._h, _stream(stream), _devptr(s), nkeys, int(p), int(x0), int(B), _devptr(out),
                                    _devptr(work)))
        return out[0] if single else out


class RLWE:
    """RLWE / RLWR instances over one plan (lol RLWE/{Continuous,Discrete,RLWR}.hs; rlwe-challenges Generate.hs:192-218,
    Verify.hs:346-366): batched sampling against one secret, error terms, their gSqNorm and the validity checks.  Arrays
    are numpy (staged through HBM, numpy out) or CUDA tensors (CUDA tensors out); samplers return CUDA tensors.  a and
    the secret are in the CRT basis ([B][n][T], [n][T]); Disc b [B][n][T] in the CRT basis, Cont b float64 [B][n] and
    RLWR b int64 [B][n] in the decoding basis.  Samples come from the ChaCha20 stream of (key, ctr + b), domains 5-7
    (include/lolhip.h): never reuse (key, ctr + b); advance ctr by B between calls."""

    DISC, CONT, RLWR = 0, 1, 2

    def __init__(self, plan: Plan):
        self.plan = plan

    # ---- helpers ----------------------------------------------------------------------------------------------------
    @staticmethod
    def _dev(x, dtype):
        """a contiguous CUDA tensor of dtype from numpy or a CUDA tensor; (host?, tensor)"""
        import torch
        host = isinstance(x, np.ndarray)
        if host:
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64 if dtype == torch.float64 else np.int64)).cuda()
        if not (x.is_cuda and x.is_contiguous() and x.dtype == dtype):
            raise TypeError(f"expected a contiguous {dtype} CUDA tensor")
        return host, x

    def _batch(self, a):
        per = self.plan.n * self.plan.T
        size = a.size if isinstance(a, np.ndarray) else a.numel()
        if size % per:
            raise ValueError(f"a is not a whole number of [n={self.plan.n}, T={self.plan.T}] polynomials")
        return size // per

    def _work(self, kind, B, device="cuda"):
        import torch
        wl = lib().lolhip_rlwe_work_len(self.plan._h, kind, int(B))
        _check(min(wl, 0))
        return torch.empty((max(wl, 1),), dtype=torch.int64, device=device)

    # ---- gSqNormDec -------------------------------------------------------------------------------------------------
    def gSqNorm(self, e, stream=None):
        """gSqNormDec (Tensor.hs:147-151) of decoding-basis coefficients [B][n] -> [B]: int64 exact or saturated at
        INT64_MAX (also for a coefficient INT64_MIN), float64 with a fixed summation order."""
        import torch
        L = lib()
        isf = (e.dtype == np.float64) if isinstance(e, np.ndarray) else (e.dtype == torch.float64)
        fn = L.lolhip_gsqnorm_f64_batch if isf else L.lolhip_gsqnorm_batch
        _check(fn(self.plan._h, None, None, None, 0))
        host, e = self._dev(e, torch.float64 if isf else torch.int64)
        if e.numel() % self.plan.n:
            raise ValueError("e is not [B][n]")
        B = e.numel() // self.plan.n
        out = torch.empty((B,), dtype=e.dtype, device=e.device)
        _check(fn(self.plan._h, _stream(stream), e.data_ptr(), out.data_ptr(), B))
        return out.cpu().numpy() if host else out

    # ---- samplers ---------------------------------------------------------------------------------------------------
    def secret(self, key=None, ctr=0, stream=None):
        """a uniform secret [n][T] in the CRT basis (Generate.hs:192-218), item ctr of domain 7"""
        import torch
        L, P = lib(), self.plan
        kb = Plan._key(key)
        rc = L.lolhip_rlwe_secret(P._h, None, kb, int(ctr), None)      # the host statuses first (INVALID: the null output)
        if rc != ERR_INVALID:
            _check(rc)
        s = torch.empty((P.n, P.T), dtype=torch.int64, device="cuda")
        _check(L.lolhip_rlwe_secret(P._h, _stream(stream), kb, int(ctr), s.data_ptr()))
        return s

    def _sample(self, kind, s_crt, B, svar, p, key, ctr, stream):
        import torch
        L, P = lib(), self.plan
        kb = Plan._key(key)
        call = lambda st, sp, a, b, w, nb: L.lolhip_rlwe_sample_batch(P._h, st, kind, int(p), sp, float(svar), kb, int(ctr),
                                                                      a, b, w, nb)
        _check(call(None, None, None, None, None, 0))
        _, s_crt = self._dev(s_crt, torch.int64)
        B = int(B)
        a = torch.empty((B, P.n, P.T), dtype=torch.int64, device=s_crt.device)
        b = torch.empty((B, P.n, P.T) if kind == self.DISC else (B, P.n),
                        dtype=torch.float64 if kind == self.CONT else torch.int64, device=s_crt.device)
        work = self._work(kind, B, s_crt.device)
        _check(call(_stream(stream), s_crt.data_ptr(), a.data_ptr(), b.data_ptr(), work.data_ptr(), B))
        return a, b

    def sampleDisc(self, s_crt, B, svar, key=None, ctr=0, stream=None):
        """B discrete samples (a, b = a s + reduce (errorRounded svar)) (Discrete.hs:38-45), both [B][n][T], CRT basis"""
        return self._sample(self.DISC, s_crt, B, svar, 0, key, ctr, stream)

    def sampleCont(self, s_crt, B, svar, key=None, ctr=0, stream=None):
        """B continuous samples (a, b = a s + reduce (tGaussian svar)) (Continuous.hs:45-54): a [B][n][1] in the CRT basis,
        b float64 [B][n] in [0, q), decoding basis"""
        return self._sample(self.CONT, s_crt, B, svar, 0, key, ctr, stream)

    def sampleRLWR(self, s_crt, B, p, key=None, ctr=0, stream=None):
        """B RLWR samples (a, b = roundedProd s a) (RLWR.hs:34-38): a [B][n][1] in the CRT basis, b [B][n] in [0, p)"""
        return self._sample(self.RLWR, s_crt, B, 1.0, p, key, ctr, stream)

    # ---- error terms and norms ----------------------------------------------------------------------------------------
    def _error(self, kind, s_crt, a, b, want_e, want_norm, stream):
        import torch
        L, P = lib(), self.plan
        call = lambda st, ap, bp, sp, e, nm, w, nb: L.lolhip_rlwe_error_batch(P._h, st, kind, ap, bp, sp, e, nm, w, nb)
        _check(call(None, None, None, None, None, None, None, 0))
        dt = torch.float64 if kind == self.CONT else torch.int64
        B = self._batch(a)
        host, a = self._dev(a, torch.int64)
        _, b = self._dev(b, dt)
        _, s_crt = self._dev(s_crt, torch.int64)
        if b.numel() != B * P.n * (P.T if kind == self.DISC else 1):
            raise ValueError("a and b are not the same number of samples")
        e = torch.empty((B, P.n), dtype=dt, device=a.device) if want_e else None
        nm = torch.empty((B,), dtype=dt, device=a.device) if want_norm else None
        work = self._work(kind, B, a.device)
        _check(call(_stream(stream), a.data_ptr(), b.data_ptr(), s_crt.data_ptr(), None if e is None else e.data_ptr(),
                    None if nm is None else nm.data_ptr(), work.data_ptr(), B))
        out = tuple(t.cpu().numpy() if host else t for t in (e, nm) if t is not None)
        return out if len(out) > 1 else out[0]

    def errorTermDisc(self, s_crt, a, b, norm=False, stream=None):
        """liftDec (b - a s) (Discrete.hs:48-52): int64 [B][n], INT64_MIN where the lift does not fit; norm=True: (e, norm)"""
        return self._error(self.DISC, s_crt, a, b, True, norm, stream)

    def errorTermCont(self, s_crt, a, b, norm=False, stream=None):
        """lift (b - a s) in K/(qR) (Continuous.hs:57-61): float64 [B][n]; norm=True: (e, norm)"""
        return self._error(self.CONT, s_crt, a, b, True, norm, stream)

    def errorGSqNormDisc(self, s_crt, a, b, stream=None):
        """gSqNorm . errorTerm (Discrete.hs:56-59): int64 [B], saturated; the error slab is not returned"""
        return self._error(self.DISC, s_crt, a, b, False, True, stream)

    def errorGSqNormCont(self, s_crt, a, b, stream=None):
        """gSqNorm . errorTerm (Continuous.hs:65-68): float64 [B]"""
        return self._error(self.CONT, s_crt, a, b, False, True, stream)

    # ---- RLWR ---------------------------------------------------------------------------------------------------------
    def roundedProd(self, s_crt, a, p, stream=None):
        """roundedProd s a (RLWR.hs:40-44): [B][n] in [0, p), decoding basis"""
        import torch
        L, P = lib(), self.plan
        _check(L.lolhip_rlwr_rounded_prod_batch(P._h, int(p), None, None, None, None, None, 0))
        B = self._batch(a)
        host, a = self._dev(a, torch.int64)
        _, s_crt = self._dev(s_crt, torch.int64)
        out = torch.empty((B, P.n), dtype=torch.int64, device=a.device)
        work = self._work(self.RLWR, B, a.device)
        _check(L.lolhip_rlwr_rounded_prod_batch(P._h, int(p), _stream(stream), a.data_ptr(), s_crt.data_ptr(),
                                                out.data_ptr(), work.data_ptr(), B))
        return out.cpu().numpy() if host else out

    def mismatchRLWR(self, s_crt, a, b, p, stream=None):
        """per sample, the coefficients where b differs from roundedProd s a: int32 [B]"""
        import torch
        L, P = lib(), self.plan
        _check(L.lolhip_rlwr_check_batch(P._h, int(p), None, None, None, None, None, None, 0))
        B = self._batch(a)
        host, a = self._dev(a, torch.int64)
        _, b = self._dev(b, torch.int64)
        _, s_crt = self._dev(s_crt, torch.int64)
        if b.numel() != B * P.n:
            raise ValueError("a and b are not the same number of samples")
        out = torch.empty((B,), dtype=torch.int32, device=a.device)
        work = self._work(self.RLWR, B, a.device)
        _check(L.lolhip_rlwr_check_batch(P._h, int(p), _stream(stream), a.data_ptr(), b.data_ptr(), s_crt.data_ptr(),
                                         out.data_ptr(), work.data_ptr(), B))
        return out.cpu().numpy() if host else out

    # ---- instance verification (Verify.hs:346-366): one copy of B values, then the comparison on the host --------------
    def validDisc(self, bound, s_crt, a, b, stream=None):
        """bound > errorGSqNorm for every sample (Verify.hs:350): bool [B]"""
        nm = self.errorGSqNormDisc(s_crt, a, b, stream)
        nm = nm if isinstance(nm, np.ndarray) else nm.cpu().numpy()
        return np.asarray(nm.astype(object) < bound, dtype=bool)       # Python integers: exact for any bound

    def validCont(self, bound, s_crt, a, b, stream=None):
        """bound > errorGSqNorm for every sample (Verify.hs:356): bool [B]"""
        nm = self.errorGSqNormCont(s_crt, a, b, stream)
        nm = nm if isinstance(nm, np.ndarray) else nm.cpu().numpy()
        return float(bound) > nm

    def validRLWR(self, s_crt, a, b, p, stream=None):
        """b == roundedProd s a for every sample (Verify.hs:362): bool [B]"""
        mm = self.mismatchRLWR(s_crt, a, b, p, stream)
        mm = mm if isinstance(mm, np.ndarray) else mm.cpu().numpy()
        return mm == 0

    @staticmethod
    def errorBound(m, svar, eps=2.0 ** -25, kind="cont"):
        """errorBound svar eps over index m (host): kind "cont" (Continuous.hs:74-84) a float, "disc" (Discrete.hs:65-76)
        an int"""
        k = {"disc": 0, "cont": 1, 0: 0, 1: 1}[kind]
        pps = factor_pps(int(m))
        arr = (_PP * max(1, len(pps)))()
        for i, (p, e) in enumerate(pps):
            arr[i].prime, arr[i].exponent = p, e
        out = C.c_double()
        _check(lib().lolhip_rlwe_error_bound(arr, len(pps), float(svar), float(eps), k, C.byref(out)))
        return int(out.value) if k == 0 else out.value
