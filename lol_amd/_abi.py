"""lol_amd/_abi.py — the C ABI of include/lolhip.h as data: status and selector constants, the error classes, the
pointer types and one table of every bound entry's return and parameter types.  tests/test_abi_host.py compares the
table and the constants with the header, so a wrong width (which ctypes would truncate silently) fails a test.
Data and the function that applies it only; the loaded library lives in lol_amd/tensor.py."""
import ctypes as C

OK, ERR_INVALID, ERR_MODULUS, ERR_NO_CRT, ERR_ROOT, ERR_NO_DEVICE, ERR_HIP, ERR_NOT_DIVISIBLE, ERR_DEVICE = 0, -1, -2, -3, -4, -5, -6, -7, -8
_ERRNAMES = {ERR_INVALID: "invalid argument", ERR_MODULUS: "modulus out of range / missing inverse",
             ERR_NO_CRT: "no CRT basis for this modulus", ERR_ROOT: "bad root of unity",
             ERR_NO_DEVICE: "no HIP device (liblolhip has no CPU fallback)", ERR_HIP: "HIP runtime error",
             ERR_NOT_DIVISIBLE: "not divisible by g",
             ERR_DEVICE: "the current HIP device is not the plan's device"}

OP_CRT, OP_CRTINV, OP_MUL, OP_POLYMUL, OP_L, OP_LINV, OP_MULGPOW, OP_MULGDEC, OP_DIVGPOW, OP_DIVGDEC, OP_MULGCRT, OP_DIVGCRT = range(12)
EXT_TWACE_POWDEC, EXT_TWACE_CRT, EXT_EMBED_POW, EXT_EMBED_DEC, EXT_EMBED_CRT, EXT_COEFFS = range(6)
ELT_I64, ELT_F64, ELT_C64 = range(3)
PLAN_DENSE_GAUSS = 1
ROUTE_DENSE_ZQ = 1
ROUTE_SCAN_ZQ = 4            # honoured by lolhip_plan_create_opts only; 2 is not defined
PLAN_DENSE_CPLX = 2          # honoured by lolhip_plan_create_opts only


class LolHipError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        super().__init__(f"lolhip: {_ERRNAMES.get(code, code)} ({code}) {what}")


class NoDeviceError(LolHipError):
    pass


def _check(rc, what=""):
    if rc == OK:
        return
    raise (NoDeviceError if rc == ERR_NO_DEVICE else LolHipError)(rc, what)


def _len(rc, what=""):
    """a count or length the library returns, a negative value being a status"""
    if rc < 0:
        _check(rc, what)
    return rc


class _PP(C.Structure):
    _fields_ = [("prime", C.c_int16), ("exponent", C.c_int16)]


class _PlanOpts(C.Structure):
    """lolhip_plan_opts"""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("routes", C.c_uint32)]


_i64p = C.POINTER(C.c_int64)
_i32p = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)

vp, i64, ci, f64, u32, u64, cstr = C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_uint32, C.c_uint64, C.c_char_p
pp, vpp, cip, f64p, u32p, u64p, u8pp = (C.POINTER(t) for t in (_PP, vp, ci, f64, u32, u64, _u8p))


def _rows(*rows):
    """(names sharing the signature, restype, parameter types ...) -> {entry: (restype, argtypes)}"""
    return {f"lolhip_{nm}": (res, list(args)) for names, res, *args in rows for nm in names.split()}


# One row per signature of include/lolhip.h; the drop-in symbols (tensorCRTRq ...) are not bound.
ABI = _rows(
    ("last_status device_count", ci),
    ("version", cstr),
    ("thread_release", None),
    ("debug_set", ci, cstr, ci),
    ("copy_slab", ci, vp, vp, vp, i64, ci),
    ("good_q", i64, i64, i64),
    # plans and the Tensor operations
    ("plan_create", ci, pp, ci, _i64p, ci, ci, vpp),
    ("plan_create_roots", ci, pp, ci, _i64p, ci, _i64p, _i64p, ci, vpp),
    ("plan_create_flags", ci, pp, ci, _i64p, ci, ci, u32, vpp),
    ("plan_gauss_route", ci, vp),
    ("plan_gauss_table", i64, vp, ci, ci, f64p, i64),
    ("plan_create_routes", ci, pp, ci, _i64p, ci, ci, u32, u32, vpp),
    ("plan_create_opts", ci, pp, ci, _i64p, ci, ci, C.POINTER(_PlanOpts), vpp),
    ("plan_cplx_route", ci, vp),
    ("plan_cplx_table", i64, vp, ci, ci, ci, f64p, i64),
    ("plan_zq_route plan_scan_route", ci, vp, ci),
    ("plan_zq_table", i64, vp, ci, ci, ci, ci, _i64p, i64),
    ("plan_destroy ext_destroy khprf_destroy tunnel_chain_destroy ptround_destroy pt_tunnel_destroy ringmul_destroy lprf_destroy", None, vp),
    ("plan_n plan_m", i64, vp),
    ("plan_T plan_has_crt", ci, vp),
    ("plan_table", i64, vp, ci, ci, _i64p, i64),
    ("crt_batch crtinv_batch l_batch linv_batch mulgpow_batch mulgdec_batch divgpow_batch divgdec_batch mulgcrt_batch "
     "divgcrt_batch crtc_batch crtinvc_batch gaussian_dec_batch", ci, vp, vp, vp, i64),
    ("mul_batch", ci, vp, vp, vp, vp, i64),
    ("polymul_batch", ci, vp, vp, vp, vp, vp, i64),
    ("op_host ext_host", ci, vp, ci, _i64p, _i64p, i64),
    ("elt_op_batch", ci, vp, vp, ci, ci, ci, vp, vp, i64),
    ("mulc_batch", ci, vp, vp, vp, i64),
    # ring extensions
    ("ext_create ringmul_create", ci, vp, vp, vpp),
    ("twace_powdec_batch twace_crt_batch embed_pow_batch embed_dec_batch embed_crt_batch coeffs_batch", ci, vp, vp, vp, vp, i64),
    ("ext_table", i64, vp, ci, _i32p, i64),
    ("evallin_batch", ci, vp, vp, vp, vp, vp, vp, vp, i64),
    ("tunnel_work_len", i64, vp, vp, i64, i64),
    ("tunnel_batch", ci, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, i64),
    # SymmSHE pipelines
    ("ctmul_crt_batch", ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64),
    ("decompose_len", ci, vp, i64),
    ("gadget", ci, vp, i64, _i64p, i64),
    ("decompose_batch", ci, vp, vp, vp, i64, vp, i64),
    ("knapsack_batch", ci, vp, vp, vp, ci, vp, ci, vp, vp, i64),
    ("keyswitch_batch", ci, vp, vp, vp, i64, vp, ci, vp, vp, vp, i64),
    ("rescale_drop_batch", ci, vp, vp, vp, vp, i64),
    ("decrypt_work_len rlwe_work_len", i64, vp, ci, i64),
    ("error_term_batch", ci, vp, vp, vp, ci, ci, vp, ci, i64, vp, vp, i64),
    ("decrypt_batch", ci, vp, vp, vp, vp, vp, ci, ci, vp, ci, i64, i64, vp, vp, i64),
    ("encrypt_work_len tunnel_chain_work_len ptround_work_len pt_tunnel_work_len ringmul_work_len", i64, vp, i64),
    ("encrypt_batch", ci, vp, vp, vp, vp, vp, vp, f64, cstr, u64, ci, vp, vp, i64),
    ("error_rounded_batch", ci, vp, vp, f64, cstr, u64, vp, vp, i64),
    ("chacha20_block", None, cstr, u32, u32p, u32p),
    ("kshint_work_len khprf_work_len", i64, vp, i64, i64),
    ("kshint_batch", ci, vp, vp, vp, vp, f64, i64, cstr, u64, vp, vp, i64),
    ("tunnel_hint_work_len public_work_len", i64, vp, vp, i64),
    ("tunnel_hint_batch", ci, vp, vp, vp, vp, vp, vp, f64, i64, cstr, u64, vp, vp),
    ("khprf_create", ci, vp, i64, _i32p, ci, _i64p, _i64p, vpp),
    ("khprf_create_lifted", ci, vp, vp, i64, _i32p, ci, _i64p, _i64p, vpp),
    ("khprf_eval_batch", ci, vp, vp, i64, i64, vp, vp),
    ("khprf_batch", ci, vp, vp, vp, ci, i64, i64, i64, vp, vp),
    ("lprf_create", ci, i64, i64, ci, _i32p, ci, _i64p, _i64p, vpp),
    ("lprf_n lprf_ell", ci, vp),
    ("lprf_work_len", i64, vp, ci, i64, i64),
    ("lprf_eval_batch", ci, vp, vp, i64, i64, vp, vp),
    ("lprf_batch", ci, vp, vp, vp, ci, i64, i64, i64, vp, vp),
    ("encode_scales", ci, vp, i64, ci, _i64p, _i64p),
    ("ct_lincomb_batch", ci, vp, vp, vp, ci, _i64p, vp, ci, _i64p, vp, i64),
    ("add_public_batch", ci, vp, vp, vp, vp, vp, i64, vp, ci, ci, ci, ci, i64, i64, i64, vp, _i64p, vp, i64),
    ("mul_public_batch", ci, vp, vp, vp, vp, i64, i64, vp, ci, ci, vp, vp, i64),
    ("modswitch_work_len", i64, vp, vp, ci, i64),
    ("modswitch_batch", ci, vp, vp, vp, vp, ci, ci, ci, i64, i64, vp, ci, _i64p, vp, i64),
    ("tunnel_chain_create", ci, ci, vpp, vpp, vpp, vpp, i64, vp, vp, vpp),
    ("tunnel_chain_batch", ci, vp, vp, vp, ci, ci, i64, i64, vp, ci, _i64p, vp, i64),
    ("ct_affine_mul_batch", ci, vp, vp, vp, _i64p, vp, vp, _i64p, vp, ci, vp, i64),
    ("ptround_create", ci, ci, i64, vpp, vpp, vpp, i64, vp, vp, vp, vpp),
    ("ptround_batch", ci, vp, vp, vp, ci, ci, i64, i64, vp, ci, _i64p, _i64p, vp, i64),
    ("ct_mul_rule", ci, vp, i64, ci, i64, i64, ci, i64, i64, _i64p, cip, _i64p, _i64p),
    ("ct_mul_work_len", i64, vp, ci, ci, ci, ci, i64),
    ("ct_mul_batch", ci, vp, vp, vp, ci, vp, ci, ci, _i64p, vp, ci, vp, i64),
    ("crtset_dec", i64, pp, ci, pp, ci, i64, _i64p, i64),
    ("crtset_modulus", i64, pp, ci, i64, ci),
    ("crtset_host", i64, pp, ci, pp, ci, i64, ci, _i64p, i64),
    ("crtset", i64, vp, pp, ci, pp, ci, i64, ci, vp, vp, i64),
    ("pt_tunnel_modulus", i64, pp, ci, pp, ci, i64, ci, i64, ci),
    ("pt_tunnel_create", ci, ci, vpp, vpp, C.POINTER(_i64p), i64, ci, vpp),
    ("pt_tunnel_batch", ci, vp, vp, vp, vp, vp, i64),
    ("ringmul_moduli", ci, pp, ci, _i64p, ci, _i64p),
    ("ringmul_batch", ci, vp, vp, vp, vp, vp, vp, i64),
    ("ringmul_prepare", ci, vp, vp, vp, vp, vp, i64),
    ("ringmul_prepared_batch", ci, vp, vp, vp, vp, vp, i64, vp, i64),
    ("gadget_correct_work_len", i64, vp, i64, ci, i64),
    ("gadget_correct_batch", ci, vp, vp, vp, i64, ci, vp, vp, vp, i64),
    ("gadget_encode_batch", ci, vp, vp, vp, i64, vp, vp, i64),
    # RLWE / RLWR
    ("gsqnorm_batch gsqnorm_f64_batch", ci, vp, vp, vp, vp, i64),
    ("rlwe_secret", ci, vp, vp, cstr, u64, vp),
    ("rlwe_sample_batch", ci, vp, vp, ci, i64, vp, f64, cstr, u64, vp, vp, vp, i64),
    ("rlwe_error_batch", ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, i64),
    ("rlwr_rounded_prod_batch", ci, vp, i64, vp, vp, vp, vp, vp, i64),
    ("rlwr_check_batch", ci, vp, i64, vp, vp, vp, vp, vp, vp, i64),
    ("rlwe_error_bound", ci, pp, ci, f64, f64, ci, f64p),
    # RLWE / RLWR over moduli without a CRT basis
    ("rlwe_ring_work_len", i64, vp, vp, ci, i64),
    ("rlwe_ring_secret", ci, vp, vp, vp, cstr, u64, vp, vp),
    ("rlwe_ring_sample_batch", ci, vp, vp, vp, ci, i64, vp, f64, cstr, u64, vp, vp, vp, i64),
    ("rlwe_ring_error_batch", ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, i64),
    ("rlwr_ring_rounded_prod_batch", ci, vp, vp, i64, vp, vp, vp, vp, vp, i64),
    ("rlwr_ring_check_batch", ci, vp, vp, i64, vp, vp, vp, vp, vp, vp, i64),
    # whole RLWE / RLWR challenges
    ("chall_work_len", i64, vp, ci, i64, i64),
    ("chall_generate_batch", ci, vp, vp, ci, i64, f64, cstr, u64, u64, i64, i64, vp, vp, vp, vp),
    ("chall_verify_batch", ci, vp, vp, ci, i64, i64, f64, i64, i64, vp, vp, vp, vp, vp, vp),
    ("chall_ring_work_len", i64, vp, vp, ci, i64, i64),
    ("chall_ring_generate_batch", ci, vp, vp, vp, ci, i64, f64, cstr, u64, u64, i64, i64, vp, vp, vp, vp),
    ("chall_ring_verify_batch", ci, vp, vp, vp, ci, i64, i64, f64, i64, i64, vp, vp, vp, vp, vp, vp),
    # serialisation (lol_amd/wire.py)
    ("rqproduct_read", i64, _u8p, i64, u32p, _i64p, ci, cip, _i64p, i64),
    ("rqproduct_write", i64, u32, _i64p, ci, _i64p, i64, _u8p, i64),
    ("kshint_read", i64, _u8p, i64, u32p, _i64p, ci, cip, cip, cip, _i64p, i64),
    ("kshint_write", i64, u32, _i64p, ci, ci, ci, _i64p, i64, u64, u64, _u8p, i64),
    ("r_read", i64, _u8p, i64, u32p, _i64p, i64),
    ("r_write", i64, u32, _i64p, i64, _u8p, i64),
    ("secretkey_read", i64, _u8p, i64, u32p, f64p, _i64p, i64),
    ("secretkey_write", i64, u32, f64, _i64p, i64, _u8p, i64),
    ("kqproduct_read", i64, _u8p, i64, u32p, _i64p, ci, cip, f64p, i64),
    ("linearrq_read", i64, _u8p, i64, u32p, u32p, cip, u32p, _i64p, ci, cip, _i64p, i64),
    ("linearrq_write", i64, u32, u32, u32, _i64p, ci, ci, _i64p, i64, _u8p, i64),
    ("tunnelhint_read", i64, _u8p, i64, u32p, u32p, u32p, u64p, _i64p, _i64p, _i64p, _i64p, ci),
    ("tunnelhint_write", i64, _u8p, i64, u8pp, _i64p, ci, u32, u32, u32, u64, _u8p, i64),
    ("chain_read", i64, _u8p, i64, _i64p, _i64p, ci),
    ("chain_write", i64, u8pp, _i64p, ci, _u8p, i64),
    # the messages of rlwe-challenges (lol_amd/challenges.py)
    ("challenge_read", i64, _u8p, i64, _i64p, cip, _i64p, f64p),
    ("challenge_write", i64, _i64p, ci, _i64p, f64p, _u8p, i64),
    ("instance_read", i64, _u8p, i64, ci, _i64p, _i64p, f64p, cip, cip, _i64p, ci, _i64p, _i64p, i64, vp, i64),
    ("instance_write", i64, ci, ci, _i64p, _i64p, f64p, _i64p, ci, i64, i64, _i64p, vp, _u8p, i64),
    ("secret_read", i64, _u8p, i64, _i64p, _i64p, _i64p, _u8p, i64, _i64p, cip, cip, _i64p, ci, _i64p, i64),
    ("secret_write", i64, ci, _i64p, i64, i64, _u8p, i64, _i64p, ci, _i64p, i64, _u8p, i64),
)


def bind(L):
    """declare every entry of ABI on the loaded library L"""
    for name, (res, args) in ABI.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L
