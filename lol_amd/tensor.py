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

The types of the C entries are the table of lol_amd/_abi.py; the protocol-buffer messages are lol_amd/wire.py.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os

import numpy as np

from ._abi import (  # noqa: F401  (the constants and types are part of this module's surface)
    OK, ERR_INVALID, ERR_MODULUS, ERR_NO_CRT, ERR_ROOT, ERR_NO_DEVICE, ERR_HIP, ERR_NOT_DIVISIBLE, ERR_DEVICE,
    OP_CRT, OP_CRTINV, OP_MUL, OP_POLYMUL, OP_L, OP_LINV, OP_MULGPOW, OP_MULGDEC, OP_DIVGPOW, OP_DIVGDEC, OP_MULGCRT,
    OP_DIVGCRT, EXT_TWACE_POWDEC, EXT_TWACE_CRT, EXT_EMBED_POW, EXT_EMBED_DEC, EXT_EMBED_CRT, EXT_COEFFS,
    ELT_I64, ELT_F64, ELT_C64, PLAN_DENSE_GAUSS, ROUTE_DENSE_ZQ, ROUTE_SCAN_ZQ, PLAN_DENSE_CPLX, LolHipError, NoDeviceError, _PP, _PlanOpts, _i64p, _i32p, _check, _len, bind)

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path() -> str:
    return os.path.join(_HERE, "liblolhip.so")


_lib = None          # the loaded library: None until lib() has run (tests/conftest.py reads it after every test)


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
    _lib = bind(C.CDLL(path))
    return _lib


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


# ---- the call protocol of the out-of-place batched entries ------------------------------------------------------------
# numpy in -> numpy out (staged through HBM with torch); CUDA tensors in -> CUDA tensors out.  The in-place operations
# (crt ... divGCRT, mul, polymul, the float members, the Ext maps) are a different contract and call the library directly.
class _Nulls:
    """the pointer lists of a dry run: every element is the null pointer"""
    def __getitem__(self, i):
        return None


def _np(a):
    a = np.ascontiguousarray(a, dtype=np.int64)
    return a, a.ctypes.data_as(_i64p)


def _ptr(t, dtype="int64"):
    """device address of a contiguous CUDA tensor of that dtype; None stays the null pointer"""
    if t is None:
        return None
    if not (t.is_cuda and t.is_contiguous() and str(t.dtype) == "torch." + dtype):
        raise TypeError(f"expected a contiguous {dtype} CUDA tensor")
    return t.data_ptr()


def _devptr(x):
    """raw device address of a torch CUDA int64 tensor, or an int address (the in-place operations' _ptr)"""
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


def _size(x):
    return x.size if isinstance(x, np.ndarray) else x.numel()


def _count(x, per, what):
    """how many items of `per` elements the array or tensor x holds; ValueError(what) unless it is a whole number"""
    size = x.size if isinstance(x, np.ndarray) else x.numel()
    B = size // max(per, 1)
    if B * per != size:
        raise ValueError(what)
    return B


def _enc(enc):
    return {"LSD": 0, "MSD": 1, 0: 0, 1: 1}[enc]


def _key(key):
    key = os.urandom(32) if key is None else bytes(key)
    if len(key) != 32:
        raise ValueError("key must be 32 bytes")
    return key


def _alloc(shape, dtype, device):
    import torch
    return torch.empty(tuple(shape), dtype=getattr(torch, dtype), device=device)


def _stage(*arrays):
    """(host?, tensors): numpy inputs (arrays[0] decides) as CUDA tensors.  An input is an array or tensor, taken as
    int64, or (array or tensor, dtype name); None stays None."""
    import torch
    pairs = [a if isinstance(a, tuple) else (a, "int64") for a in arrays]
    host = isinstance(pairs[0][0], np.ndarray)
    return host, [x if x is None or not host else torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda()
                  for x, dt in pairs]


def _unstage(host, *tensors):
    out = tuple(t.cpu().numpy() if host and t is not None else t for t in tensors)
    return out if len(out) > 1 else out[0]


def _dry(call, tolerate=()):
    """The dry run of a batched entry: B = 0 and null pointers, so every host status is raised before anything touches
    the device.  _run makes it first; an entry whose own shape checks come after it calls it itself."""
    rc = call(None, _Nulls(), _Nulls(), None, 0)
    if rc not in tolerate:
        _check(rc)


def _run(call, stream, inputs, B, work_len, outs, out=None, dry=True, unstage=True, min_work=1):
    """The protocol of the batched entries.  call(stream, i, o, work, B) wraps one C entry, i and o being the lists of
    its input and output pointers (host scalars it returns go through `byref` in the closure).  First the dry run (_dry;
    not with dry=False); then numpy inputs (inputs[0] decides) are staged, the work buffer (work_len() int64 words, at
    least min_work; None: the entry has none) and the outputs allocated, the real call made and the outputs unstaged
    (unstage=False: they stay CUDA tensors).  An input is as for _stage, each checked contiguous, CUDA and of its dtype;
    None is the null pointer.  outs() gives the shape of one int64 output, or a list of (shape, dtype name) per output,
    None for an output not asked for, and the result is one output or the list.  `out` replaces the first output."""
    if dry:
        _dry(call)
    dts = [a[1] if isinstance(a, tuple) else "int64" for a in inputs]
    host, dev = _stage(*inputs) if inputs else (False, [])
    device = dev[0].device if dev else "cuda"
    work = None if work_len is None else _alloc((max(_len(work_len()), min_work),), "int64", device)
    specs = outs()
    single = isinstance(specs, tuple)
    specs = [(specs, "int64")] if single else specs
    res = [None if s is None else _alloc(*s, device) if out is None or k else out for k, s in enumerate(specs)]
    _check(call(_stream(stream), [_ptr(t, dt) for t, dt in zip(dev, dts)],
                [None if s is None else _ptr(t, s[1]) for t, s in zip(res, specs)], _ptr(work), B))
    res = [t.cpu().numpy() if host and unstage and t is not None else t for t in res]
    return res[0] if single else res


class _Handle:
    """Owner of one library object: `_h`, made by lolhip_<_kind>_create... and given back once to
    lolhip_<_kind>_destroy."""
    _kind = None

    def _create(self, entry, *args, what=""):
        h = C.c_void_p()
        _check(getattr(lib(), f"lolhip_{entry}")(*args, C.byref(h)), what or entry)
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None       # no _h: the constructor raised before it made the object
        if h and _lib is not None:
            getattr(_lib, f"lolhip_{self._kind}_destroy")(h)


class _WorkHandle(_Handle):
    """a handle with a lolhip_<_kind>_work_len entry"""

    def workLen(self, B):
        return _len(getattr(lib(), f"lolhip_{self._kind}_work_len")(self._h, int(B)))


def crtSetDec(pps_m, pps_m2, p):
    """crtSetDec (CPP/Extension.hs:143-164) on the host: the mod-p CRT set of O_m'/O_m as [K][phi(m')] residues in
    [0, p), decoding basis of O_m'.  pps_m, pps_m2: prime-power lists [(p, e)] or the indices themselves; p: a prime
    that does not divide m'.  Order and root of unity: include/lolhip.h."""
    (_, a, na), (pps2, b, nb) = _pps(pps_m), _pps(pps_m2)
    L = lib()
    K = _len(L.lolhip_crtset_dec(a, na, b, nb, int(p), None, 0), f"crtSetDec(p={p})")
    out = np.zeros((K, _totient(pps2)), dtype=np.int64)
    _len(L.lolhip_crtset_dec(a, na, b, nb, int(p), out.ctypes.data_as(_i64p), K), f"crtSetDec(p={p})")
    return out


def crtSet(pps_m, pps_m2, p, e, host=False, stream=None):
    """crtSet (UCyc.hs:540-565): the mod-p^e CRT set of O_m'/O_m as [K][phi(m')] residues in [0, p^e), powerful basis
    of O_m'.  On the device (a CUDA tensor; lolhip_crtset over a plan of the p-free part of m' mod the NTT prime of
    lolhip_crtset_modulus), or with host=True by schoolbook products on the host (numpy; small indices)."""
    (_, a, na), (pps2, b, nb) = _pps(pps_m), _pps(pps_m2)
    L, n2, what = lib(), _totient(pps2), f"crtSet(p={p}, e={e})"
    if host:
        K = _len(L.lolhip_crtset_host(a, na, b, nb, int(p), int(e), None, 0), what)
        out = np.zeros((K, n2), dtype=np.int64)
        _len(L.lolhip_crtset_host(a, na, b, nb, int(p), int(e), out.ctypes.data_as(_i64p), K), what)
        return out
    import torch
    if all(q[0] == int(p) for q in pps2):
        # m' is a power of p: its p-free part is the index 1, the set is {1}; nothing to run on the device
        return torch.from_numpy(crtSet(pps_m, pps_m2, p, e, host=True)).cuda()
    plan = Plan([q for q in pps2 if q[0] != int(p)], [_len(L.lolhip_crtset_modulus(b, nb, int(p), int(e)), what)])
    K = _len(L.lolhip_crtset(plan._h, a, na, b, nb, int(p), int(e), None, None, 0), what)   # the statuses and the count
    # no dry run: the count query above is this entry's; it returns a count, of which only a status is an error
    return _run(lambda st, i, o, w, k: min(L.lolhip_crtset(plan._h, a, na, b, nb, int(p), int(e), st, o[0], k), 0),
                stream, (), K, None, lambda: (K, n2), dry=False)


class Plan(_Handle):
    """Twiddles, g vectors, stage programs and moduli for one (m, moduli), resident in HBM.

    Mirrors what lol-cpp's shim marshals per call: `ru`/`ruInv` (CPP.hs:422-442),
    `mhatInv` (ZqBasic.hs:167-171), `gCRT`/`gInvCRT` (CPP.hs:444-454), the prime-power
    list (CPP.hs:325-337) and the moduli (Backend.hs:195-199)."""
    _kind = "plan"

    def __init__(self, pps, qs, host_only=False, omega_pp=None, mhatinv=None, dense_gauss=False, dense_zq=False, dense_cplx=False, scan_zq=False):
        """dense_gauss: the Gaussian map (gaussianDec and every sampler behind it) also takes primes above 13, as dense
        stages (LOLHIP_PLAN_DENSE_GAUSS; default roots only).  dense_zq: crt, crtInv and what is composed of them run the
        stages of a prime above 13 as dense products out of an LDS tile (LOLHIP_ROUTE_DENSE_ZQ; default roots only): the
        same residues from another kernel.  dense_cplx: crtC / crtInvC also take primes above 13 (up to 1021), as dense
        stages on the FP64 matrix cores or the vector ALU (LOLHIP_PLAN_DENSE_CPLX, lolhip_plan_create_opts; default roots
        only; cplxRoute() says whether the index is served).  scan_zq: L, LInv, mulGPow/Dec and divGPow/Dec over Z_q run
        the stages of a prime above 13 as scans on an LDS tile (LOLHIP_ROUTE_SCAN_ZQ, lolhip_plan_create_opts; default
        roots only; needs no CRT basis; scanRoute(op) says which ops take it): the same residues from another kernel.
        The four compose."""
        self.pps, arr, npp = _pps(list(pps))
        self.qs = [int(q) for q in qs]
        self.host_only = bool(host_only)
        qa = (C.c_int64 * len(self.qs))(*self.qs)
        what = f"plan_create(pps={self.pps}, qs={self.qs})"
        if dense_cplx or scan_zq:
            if omega_pp is not None or mhatinv is not None:
                raise ValueError(f"{'dense_cplx' if dense_cplx else 'scan_zq'} plans take the default roots")
            opts = _PlanOpts(C.sizeof(_PlanOpts), (PLAN_DENSE_GAUSS if dense_gauss else 0) | (PLAN_DENSE_CPLX if dense_cplx else 0),
                             (ROUTE_DENSE_ZQ if dense_zq else 0) | (ROUTE_SCAN_ZQ if scan_zq else 0))
            self._create("plan_create_opts", arr, npp, qa, len(self.qs), int(host_only), C.byref(opts), what=what)
        elif dense_zq:
            if omega_pp is not None or mhatinv is not None:
                raise ValueError("dense_zq plans take the default roots")
            self._create("plan_create_routes", arr, npp, qa, len(self.qs), int(host_only),
                         PLAN_DENSE_GAUSS if dense_gauss else 0, ROUTE_DENSE_ZQ, what=what)
        elif dense_gauss:
            if omega_pp is not None or mhatinv is not None:
                raise ValueError("dense_gauss plans take the default roots")
            self._create("plan_create_flags", arr, npp, qa, len(self.qs), int(host_only), PLAN_DENSE_GAUSS, what=what)
        elif omega_pp is None and mhatinv is None:
            self._create("plan_create", arr, npp, qa, len(self.qs), int(host_only), what=what)
        else:
            om = None if omega_pp is None else (C.c_int64 * len(omega_pp))(*[int(v) for v in omega_pp])
            mh = None if mhatinv is None else (C.c_int64 * len(mhatinv))(*[int(v) for v in mhatinv])
            self._create("plan_create_roots", arr, npp, qa, len(self.qs), om, mh, int(host_only), what=what)
        L, h = lib(), self._h
        self.n = int(L.lolhip_plan_n(h))
        self.m = int(L.lolhip_plan_m(h))
        self.T = int(L.lolhip_plan_T(h))
        self.has_crt = bool(L.lolhip_plan_has_crt(h))
        self.dense_gauss = bool(dense_gauss)
        self.dense_zq = bool(dense_zq)
        self.dense_cplx = bool(dense_cplx)
        self.scan_zq = bool(scan_zq)

    @classmethod
    def for_index(cls, m, qs, **kw):
        return cls(factor_pps(m), qs, **kw)

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

    def gaussRoute(self):
        """How gaussianDec runs on this plan: 0 refused, 1 register stages only, 2 with a dense stage."""
        return int(lib().lolhip_plan_gauss_route(self._h))

    def gaussTable(self, k, transposed=False):
        """The (p-1) x (p-1) matrix of tensorGaussianDec for prime power k as the plan stores it: row-major, or the
        transposed copy the dense stage reads (empty unless that prime takes the dense stage)."""
        L = lib()
        cnt = L.lolhip_plan_gauss_table(self._h, k, int(transposed), None, 0)
        out = np.zeros(cnt, dtype=np.float64)
        if cnt:
            L.lolhip_plan_gauss_table(self._h, k, int(transposed), out.ctypes.data_as(C.POINTER(C.c_double)), cnt)
        d = int(round(cnt ** 0.5))
        return out.reshape(d, d)

    def cplxRoute(self):
        """How crtC / crtInvC run on this plan: 0 refused, 1 register stages only, 2 at least one dense stage."""
        return int(lib().lolhip_plan_cplx_route(self._h))

    def cplxProgram(self, inverse=False):
        """The stage program of crtC / crtInvC: rows (kind, prime, length, stride, route), route 0 a register stage or a
        diagonal, 1 dense on the vector ALU, 2 dense on the matrix cores.  No rows when cplxRoute() is 0."""
        return self._table(21 if inverse else 20).reshape(-1, 5)

    def cplxTable(self, stage, form, inverse=False):
        """A dense stage's matrix as the device reads it: form 0 the transposed copy (complex [d][d], entry [c][row]),
        forms 1, 2, 3 the planes M_re, M_im, -M_im, padded to multiples of 16 rows and 4 columns.  Empty for a stage that
        is not dense on this plan."""
        L = lib()
        cnt = L.lolhip_plan_cplx_table(self._h, int(inverse), int(stage), int(form), None, 0)
        out = np.zeros(cnt, dtype=np.float64)
        if cnt:
            L.lolhip_plan_cplx_table(self._h, int(inverse), int(stage), int(form), out.ctypes.data_as(C.POINTER(C.c_double)), cnt)
        if form == 0:
            d = int(round((cnt // 2) ** 0.5))
            return out.view(np.complex128).reshape(d, d)
        return out

    def zqRoute(self, what=0):
        """Which kernel a lone crt (what=0), a lone crtInv (1) or the poly-mul (2) launches: 0 what a plan without dense_zq
        launches, 1 the dense stages on the vector ALU, 2 on the matrix cores.  For the poly-mul 0 also means composed of
        lone transforms, which may themselves be dense."""
        return int(lib().lolhip_plan_zq_route(self._h, int(what)))

    def scanRoute(self, op):
        """Whether the scan kernel runs prime op `op` (OP_L ... OP_DIVGDEC) on this plan: 1, or 0 - what a plan without
        scan_zq launches."""
        return int(lib().lolhip_plan_scan_route(self._h, int(op)))

    def zqTable(self, stage, t=0, limb=-1, inverse=False):
        """A dense stage's matrix as the device reads it, for stage `stage` of program(inverse) and component t: the
        transposed word matrix [d][d] (limb=-1) or int8 limb plane `limb`, padded shape included.  Empty for a stage that
        is not dense on this plan."""
        L = lib()
        cnt = L.lolhip_plan_zq_table(self._h, int(inverse), int(stage), int(t), int(limb), None, 0)
        out = np.zeros(cnt, dtype=np.int64)
        if cnt:
            L.lolhip_plan_zq_table(self._h, int(inverse), int(stage), int(t), int(limb), out.ctypes.data_as(_i64p), cnt)
        d = int(round(cnt ** 0.5))
        return out.reshape(d, d)

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
        """how many [n][T] polynomials the array or tensor holds"""
        return _count(a, self.n * self.T, "not a whole number of [n][T] polynomials of the plan")

    def _host(self, op, y, b=None):
        y = _np(y)[0].copy()
        B = self._batch(y)
        bp = None
        if b is not None:
            b, bp = _np(b)
            if b.size != y.size:
                raise ValueError("operand shapes differ")
        rc = lib().lolhip_op_host(self._h, op, y.ctypes.data_as(_i64p), bp, B)
        if rc == ERR_NOT_DIVISIBLE:
            return None
        _check(rc)
        return y

    def _dev(self, name, y, stream):
        rc = getattr(lib(), f"lolhip_{name}_batch")(self._h, _stream(stream), _devptr(y), self._batch(y))
        if rc == ERR_NOT_DIVISIBLE:
            return None
        _check(rc)
        return y

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
        _check(lib().lolhip_mul_batch(self._h, _stream(stream), _devptr(a), _devptr(b), self._batch(a)))
        return a

    def polymul(self, a, b, out=None, stream=None):
        """crtInv(crt a * crt b): one ring product per batch item, powerful basis in and out."""
        if isinstance(a, np.ndarray):
            return self._host(OP_POLYMUL, a, b)
        out = a if out is None else out
        _check(lib().lolhip_polymul_batch(self._h, _stream(stream), _devptr(out), _devptr(a), _devptr(b), self._batch(a)))
        return out

    # ---- floating-point members: float64, tolerance contract -----------
    def _float_op(self, name, y, complex_):
        """numpy in -> numpy out (staged through HBM); torch CUDA tensor -> in place."""
        dt = "complex128" if complex_ else "float64"
        host, (t,) = _stage((y, dt))
        ptr = _ptr(t, dt)
        B = _count(t, self.n, "tensor is not a whole number of polynomials")
        _check(getattr(lib(), f"lolhip_{name}_batch")(self._h, _stream(None), ptr, B))
        return _unstage(host, t)

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
        dt = str(y.dtype).replace("torch.", "")
        elt = self._ELT.get(dt)
        if elt is None:
            raise TypeError("expected an int64, float64 or complex128 array or CUDA tensor")
        if T is None:
            T = int(y.shape[-1]) if len(y.shape) >= 2 and y.shape[-2] == self.n else 1
        call = lambda st, i, o, w, b: lib().lolhip_elt_op_batch(self._h, st, int(op), elt, int(T), i[0], o[0], b)
        _dry(call)
        # in place, so not _run: the staged copy of a numpy slab (or the caller's tensor) is input and output
        host, (t,) = _stage((y, dt))
        ptr = _ptr(t, dt)
        B = _count(t, self.n * T, f"slab is not a whole number of [n={self.n}, T={T}] polynomials")
        divi = elt == ELT_I64 and op in (OP_DIVGPOW, OP_DIVGDEC)
        ok = _alloc((max(B, 1),), "int32", t.device)[:B] if divi else None
        _check(call(_stream(stream), [ptr], [ok.data_ptr() if divi else None], None, B), "elt_op")
        return _unstage(host, t, ok) if divi else _unstage(host, t)

    def lR(self, y, T=None, stream=None): return self.eltOp(OP_L, y, T, stream)
    def lInvR(self, y, T=None, stream=None): return self.eltOp(OP_LINV, y, T, stream)
    def mulGPowR(self, y, T=None, stream=None): return self.eltOp(OP_MULGPOW, y, T, stream)
    def mulGDecR(self, y, T=None, stream=None): return self.eltOp(OP_MULGDEC, y, T, stream)
    def divGPowR(self, y, T=None, stream=None): return self.eltOp(OP_DIVGPOW, y, T, stream)
    def divGDecR(self, y, T=None, stream=None): return self.eltOp(OP_DIVGDEC, y, T, stream)

    # ---- ring-level pipelines of SymmSHE (include/lolhip.h) -----------
    # ctMulCRT, decompose, knapsack, keySwitch and rescaleDropFirst make no dry run (dry=False): the first error their
    # callers see is the one the single call raises after staging, and a dry run would put a library status in front of it.
    def ctMulCRT(self, c0, c1, d0, d1, stream=None):
        """(g c0 d0, g (c0 d1 + c1 d0), g c1 d1): mulG <$> c*d for two linear ciphertexts, every
        operand in the CRT basis (SymmSHE.hs:444-449)."""
        L = lib()
        return tuple(_run(lambda st, i, o, w, b: L.lolhip_ctmul_crt_batch(self._h, st, *i, *o, b), stream,
                          (c0, c1, d0, d1), self._batch(c0), None, lambda: [(c0.shape, "int64")] * 3, dry=False))

    def decomposeLen(self, base):
        return _len(lib().lolhip_decompose_len(self._h, int(base)))

    def gadget(self, base):
        """gadget vector [L][T] (Gadget.hs:92-94 over ZqBasic.hs:227-229,248-253)."""
        out = np.zeros((self.decomposeLen(base), self.T), dtype=np.int64)
        _len(lib().lolhip_gadget(self._h, int(base), out.ctypes.data_as(_i64p), out.size))
        return out

    def decompose(self, c, base, stream=None):
        """powerful-basis c [B][n][T] -> reduced digit polynomials [L][B][n][T] (Cyc.hs:592-604)."""
        L, B = lib(), self._batch(c)
        return _run(lambda st, i, o, w, b: L.lolhip_decompose_batch(self._h, st, i[0], int(base), o[0], b), stream,
                    (c,), B, None, lambda: (self.decomposeLen(base), B, self.n, self.T), dry=False)

    _BASIS = {"dec": 0, "pow": 1, "crt": 2, 0: 0, 1: 1, 2: 2}

    def gadgetEncode(self, s, base, e=None, stream=None):
        """Gadget.encode plus noise (Gadget.hs:47-56): out_j = g_j s + reduce (e_j) for s [B][n][T] and integer errors
        e [L][B][n] (None: no noise) -> [L][B][n][T], L = decomposeLen(base); s and e in one basis, any."""
        Lb = lib()
        call = lambda st, i, o, w, b: Lb.lolhip_gadget_encode_batch(self._h, st, i[0], int(base), i[1], o[0], b)
        _dry(call)                                                   # before the shape checks
        B, L = self._batch(s), self.decomposeLen(base)
        if e is not None and _size(e) != L * B * self.n:
            raise ValueError(f"errors are not [L={L}][B={B}][n={self.n}]")
        return _run(call, stream, (s, e), B, None, lambda: (L, B, self.n, self.T), dry=False)

    def gadgetCorrectWorkLen(self, base, basis="dec", B=1):
        return _len(lib().lolhip_gadget_correct_work_len(self._h, int(base), self._BASIS[basis], int(B)))

    def gadgetCorrect(self, xs, base, basis="dec", errors=True, stream=None):
        """Gadget error correction (Correct gad (Cyc t m zq), Cyc.hs:615-621): xs [L][B][n][T], the noisy multiples
        g_j s + e_j in `basis` ("dec", "pow" or "crt") -> (u [B][n][T], es [L][B][n] int64), both in the decoding basis;
        es is None with errors=False.  T = 1 or 2; defined for every input."""
        L, bs, lb = self.decomposeLen(base), self._BASIS[basis], lib()
        call = lambda st, i, o, w, b: lb.lolhip_gadget_correct_batch(self._h, st, i[0], int(base), bs, o[0], o[1], w, b)
        _dry(call)                                                   # before the shape check
        B = _count(xs, max(L, 1) * self.n * self.T, f"xs is not [L={L}][B][n={self.n}][T={self.T}]")
        u, es = _run(call, stream, (xs,), B, lambda: self.gadgetCorrectWorkLen(base, basis, B),
                     lambda: [((B, self.n, self.T), "int64"), ((L, B, self.n), "int64") if errors else None], dry=False)
        return u, es

    def knapsack(self, xs_crt, hint, addend=None, stream=None):
        """sum_j xs_j *>> hint_j (+ addend), CRT basis (SymmSHE.hs:302-304): xs [L][B][n][T],
        hint [L][K][n][T] -> [K][B][n][T]."""
        Lb, L, K = lib(), xs_crt.shape[0], hint.shape[1]
        B = self._batch(xs_crt) // max(L, 1)
        return _run(lambda st, i, o, w, b: Lb.lolhip_knapsack_batch(self._h, st, i[0], L, i[1], K, i[2], o[0], b), stream,
                    (xs_crt, hint, addend), B, None, lambda: (K, B, self.n, self.T), dry=False)

    def keySwitch(self, c2_pow, base, hint, addend=None, stream=None):
        """addend + knapsack hint (crt (reduce <$> decompose c2)) — `switch`, SymmSHE.hs:312-314."""
        Lb, B, K = lib(), self._batch(c2_pow), hint.shape[1]
        return _run(lambda st, i, o, w, b: Lb.lolhip_keyswitch_batch(self._h, st, i[0], int(base), i[1], K, i[2], o[0], w, b),
                    stream, (c2_pow, hint, addend), B, lambda: self.decomposeLen(base) * B * self.n * self.T,   # the digits
                    lambda: (K, B, self.n, self.T), dry=False)

    def rescaleDropFirst(self, c, stream=None):
        """RescaleCyc (a,b) -> b (Cyc.hs:529-542): [B][n][T] -> [B][n][T-1]."""
        L, B = lib(), self._batch(c)
        return _run(lambda st, i, o, w, b: L.lolhip_rescale_drop_batch(self._h, st, i[0], o[0], b), stream, (c,), B, None,
                    lambda: (B, self.n, self.T - 1), dry=False)

    # ---- errorTerm / decrypt (lol-apps SymmSHE.hs:153-178) ------------------------------
    def errorTerm(self, cs, s_crt, p, enc="LSD", cs_crt=False, stream=None):
        """liftCyc Dec (evaluate c s) after toLSD (SymmSHE.hs:153-157): ciphertext components cs (a list of [B][n][T]
        or one [ncs][B][n][T] array; powerful basis, or CRT basis with cs_crt), secret key s_crt [n][T] in the CRT
        basis -> [B][n] int64 centred lifts mod Q (INT64_MIN where the lift does not fit)."""
        L = lib()
        _, cs, ncs, B = self._cs(cs)
        e = _enc(enc)
        return _run(
            lambda st, i, o, w, b: L.lolhip_error_term_batch(self._h, st, i[0], ncs, int(cs_crt), i[1], e, int(p), o[0], w, b),
            stream, (cs, s_crt), B, lambda: L.lolhip_decrypt_work_len(self._h, ncs, B), lambda: (B, self.n))

    def decrypt(self, cs, s_crt, pp, ext=None, enc="LSD", k=0, l=1, cs_crt=False, stream=None):
        """SymmSHE decrypt (SymmSHE.hs:169-174): l' twace (divG^k (reduce_p (errorTerm))).  pp: the Plan of index m' over
        the plaintext modulus p alone; ext: an Ext from the Plan of (m, p) to pp, or None for m = m'.  Returns [B][n_m]
        residues mod p in the powerful basis of R_m."""
        L = lib()
        _, cs, ncs, B = self._cs(cs)
        e, xh = _enc(enc), (None if ext is None else ext._h)
        n_out = pp.n if ext is None else ext.lo.n
        return _run(
            lambda st, i, o, w, b: L.lolhip_decrypt_batch(self._h, pp._h, xh, st, i[0], ncs, int(cs_crt), i[1], e, int(k),
                                                           int(l), o[0], w, b),
            stream, (cs, s_crt), B, lambda: L.lolhip_decrypt_work_len(self._h, ncs, B), lambda: (B, n_out))

    # ---- encrypt / genSK (lol-apps SymmSHE.hs:120-146) -------------------------------------
    def encrypt(self, pt, s_crt, pp, svar, key=None, ctr=0, ext=None, out_crt=False, stream=None):
        """SymmSHE encrypt (SymmSHE.hs:138-146) of B plaintexts pt [B][n_m] (in (-p, p), powerful basis of R_m) under
        the key s_crt [n][T] (CRT basis) -> [2][B][n][T] = (c0, c1) of CT LSD 0 1, powerful basis or the CRT basis with
        out_crt.  pp: the Plan of index m' over p alone; ext: an Ext from the Plan of (m, p) to pp, or None for m = m'.
        Samples from the ChaCha20 stream of (key, ctr + b) (include/lolhip.h); key None draws a fresh one.  Never reuse
        (key, ctr + b): advance ctr by B between calls."""
        L = lib()
        kb, xh = _key(key), (None if ext is None else ext._h)
        B = _count(pt, pp.n if ext is None else ext.lo.n, "pt is not [B][n_m]")
        return _run(
            lambda st, i, o, w, b: L.lolhip_encrypt_batch(self._h, pp._h, xh, st, i[0], i[1], float(svar), kb, int(ctr),
                                                           int(out_crt), o[0], w, b),
            stream, (pt, s_crt), B, lambda: L.lolhip_encrypt_work_len(self._h, B), lambda: (2, B, self.n, self.T))

    def errorRounded(self, svar, B=1, key=None, ctr=0, stream=None):
        """errorRounded svar (UCyc.hs:422-429; genSK, SymmSHE.hs:120-122): [B][n] int64 decoding-basis coefficients,
        from the ChaCha20 stream of (key, ctr + b); key None draws a fresh one."""
        L, kb = lib(), _key(key)
        return _run(lambda st, i, o, w, b: L.lolhip_error_rounded_batch(self._h, st, float(svar), kb, int(ctr), o[0], None, b),
                    stream, (), int(B), None, lambda: (int(B), self.n))

    # ---- key-switch hints (lol-apps SymmSHE.hs:262-296, 330-355) -------------------------
    def ksHint(self, s_crt, vals_crt, svar, base, key=None, ctr=0, stream=None):
        """ksHint skout val (SymmSHE.hs:286-296) for B values vals_crt [B][n][T] (CRT basis) under the key s_crt [n][T]
        (CRT basis) -> [B][L][2][n][T] CRT-basis hints; [b] is the hint keySwitch takes.  Row j of item b is LWE sample
        ctr + b L + j of the ChaCha20 stream (include/lolhip.h): advance ctr by B L between calls; key None draws a
        fresh key."""
        L, kb = lib(), _key(key)
        B = _count(vals_crt, self.n * self.T, "vals_crt is not [B][n][T]")
        return _run(
            lambda st, i, o, w, b: L.lolhip_kshint_batch(self._h, st, i[1], i[0], float(svar), int(base), kb, int(ctr),
                                                          o[0], w, b),
            stream, (vals_crt, s_crt), B, lambda: L.lolhip_kshint_work_len(self._h, int(base), B),
            lambda: (B, self.decomposeLen(base), 2, self.n, self.T))

    def ksLinearHint(self, s_out_crt, s_in_crt, svar, base, key=None, ctr=0, stream=None):
        """ksLinearHint skout skin (SymmSHE.hs:330-335) = ksHint skout s_in: one [L][2][n][T] hint."""
        return self.ksHint(s_out_crt, s_in_crt, svar, base, key=key, ctr=ctr, stream=stream)[0]

    def ksQuadCircHint(self, s_crt, svar, base, key=None, ctr=0, stream=None):
        """ksQuadCircHint sk (SymmSHE.hs:352-355) = ksHint sk (s*s), s*s formed on the device: one [L][2][n][T] hint."""
        # ksHint's dry run, made here as well so that it comes before the key is staged and squared
        _dry(lambda st, i, o, w, b: lib().lolhip_kshint_batch(self._h, st, i[0], i[1], float(svar), int(base), _key(key),
                                                              int(ctr), o[0], w, b))
        host, (s_crt,) = _stage(s_crt)
        s2 = s_crt.clone().contiguous()
        self.mul(s2, s_crt, stream=stream)
        return _unstage(host, self.ksHint(s_crt, s2, svar, base, key=key, ctr=ctr, stream=stream)[0])

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
        if isinstance(cs, (list, tuple)):
            if isinstance(cs[0], np.ndarray):
                cs = np.stack([np.asarray(c, dtype=np.int64) for c in cs])
            else:
                import torch
                cs = torch.stack(list(cs))
        ncs = int(cs.shape[0])
        return isinstance(cs, np.ndarray), cs, ncs, _count(cs, ncs * self.n * self.T, "cs is not [ncs][B][n][T]")

    def _per_mod(self, v):
        v = [int(v)] * self.T if np.ndim(v) == 0 else [int(x) for x in v]
        if len(v) != self.T:
            raise ValueError("expected one scalar per modulus")
        return (C.c_int64 * self.T)(*v)

    def ctLinComb(self, a, alpha, b=None, beta=None, out=None, stream=None):
        """out_i = alpha_t a_i + beta_t b_i mod q_t, i < max(na, nb), a missing component counting as zero
        (lolhip_ct_lincomb_batch); alpha, beta: an int or one int per modulus.  Either basis; out may be a or b."""
        _, a, na, B = self._cs(a)
        nb = 0
        if b is not None:
            _, b, nb, Bb = self._cs(b)
            if Bb != B:
                raise ValueError("batch sizes differ")
        al = self._per_mod(alpha)
        be = self._per_mod(0 if beta is None else beta) if b is not None else None
        L = lib()
        # the entry refuses a null b beside nb > 0 even at B = 0: the dry run names an address that is never read
        return _run(lambda st, i, o, w, n: L.lolhip_ct_lincomb_batch(self._h, st, i[0], na, al,
                                                                      None if b is None else (i[1] or 1), nb, be, o[0], n),
                    stream, (a, b), B, None, lambda: (max(na, nb), B, self.n, self.T), out=out)

    @staticmethod
    def _decode(v, p):
        """decode' (ZqBasic.hs:92-94): v mod p lifted to [-p/2, p/2)"""
        v = int(v) % int(p)
        return v - p if 2 * v >= p else v

    def toMSD(self, cs, p, enc="LSD", l=1, stream=None):
        """toMSD (SymmSHE.hs:214-222) -> (cs, "MSD", l)"""
        if _enc(enc) == 1:
            return cs, "MSD", int(l) % p
        zq, zp = self.encodeScales(p, True)
        return self.ctLinComb(cs, zq, stream=stream), "MSD", int(l) * zp % p

    def toLSD(self, cs, p, enc="MSD", l=1, stream=None):
        """toLSD (SymmSHE.hs:224-230) -> (cs, "LSD", l)"""
        if _enc(enc) == 0:
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
        host, (cs,) = _stage(self._cs(cs)[1])
        y = cs.clone()
        self._dev("mulgcrt" if cs_crt else "mulgpow", y, stream)       # in place on the copy; no dry run
        return _unstage(host, y), int(k) + 1

    def ctAdd(self, ct1, ct2, p, cs_crt=False, stream=None):
        """(+) (SymmSHE.hs:420-436) of ct = (cs, enc, k, l), aligned as the reference does, in order: l1 != l2 ->
        mulScalar (l1 / l2) on ct1; unequal k -> mulGCT on the smaller; unequal encodings -> toMSD of the LSD one; then
        the componentwise sum (the shorter one padded with zeros).  Returns (cs, enc, k, l)."""
        (c1, e1, k1, l1), (c2, e2, k2, l2) = ct1, ct2
        e1, e2, l1, l2 = _enc(e1), _enc(e2), int(l1) % p, int(l2) % p
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
        size = _size(v)
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
        args = (int(cs_shared), int(cs_crt), _enc(enc), int(k), int(l), int(p))
        out = _run(
            lambda st, i, o, w, nb: L.lolhip_add_public_batch(self._h, xh, pph, st, i[1], stride, i[0], ncs, *args, o[0],
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
        return _run(
            lambda st, i, o, w, b: L.lolhip_mul_public_batch(self._h, xh, st, i[1], stride, int(p), i[0], ncs,
                                                              int(cs_shared), o[0], w, b),
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
        args = (ncs, int(cs_crt), _enc(enc), int(l), int(p))
        out = _run(
            lambda st, i, o, w, b: L.lolhip_modswitch_batch(self._h, to._h, st, i[0], *args, o[0], int(out_crt),
                                                             C.byref(lo), w, b),
            stream, (cs,), B, lambda: L.lolhip_modswitch_work_len(self._h, to._h, ncs, B), lambda: (ncs, B, to.n, to.T))
        return out, "MSD", int(lo.value)

    def ctAffineMul(self, a, alpha, b=None, beta=1, va=None, vb=None, npairs=1, out=None, stream=None):
        """The ciphertext product with both affine pre-steps folded in (lolhip_ct_affine_mul_batch), CRT basis: for every
        pair j, (g A0 B0, g (A0 B1 + A1 B0), g A1 B1) with A0 = alpha a_0 + va_j, A1 = alpha a_1, B0 = beta b_0 + vb_j,
        B1 = beta b_1.  a, b [2][B][n][T] (b None: b = a, read once); alpha, beta: an int or one int per modulus; va, vb
        [npairs][n][T] or None -> [npairs][3][B][n][T].  With npairs = 1, out may be a or b."""
        _, a, na, B = self._cs(a)
        if b is not None:
            _, b, nb, Bb = self._cs(b)
            if Bb != B or nb != 2:
                raise ValueError("b is not a linear ciphertext of a's batch")
        if na != 2:
            raise ValueError("a is not a linear ciphertext [2][B][n][T]")
        al, be, L, npairs = self._per_mod(alpha), self._per_mod(beta), lib(), int(npairs)
        call = lambda st, i, o, w, n: L.lolhip_ct_affine_mul_batch(self._h, st, i[0], al, i[2], i[0] if b is None else i[1],
                                                                    be, i[3], npairs, o[0], n)
        _dry(call)                                                   # before the shape check of va and vb
        for v in (va, vb):
            if v is not None and _size(v) != npairs * self.n * self.T:
                raise ValueError("va / vb are not [npairs][n][T]")
        return _run(call, stream, (a, b, va, vb), B, None, lambda: (npairs, 3, B, self.n, self.T), out=out, dry=False)

    # ---- the ciphertext product (*) of any degree and the ciphertext-level key switches (SymmSHE.hs:339-371, 438-452) --
    def ctMulRule(self, p, enc1, k1, l1, enc2, k2, l2):
        """The rule of (*) (SymmSHE.hs:444-452), host only -> (alpha, enc, k, l): both MSD -> toLSD on the first operand
        (alpha_t = p mod q_t, l1 (-Q)^-1), else alpha_t = 1; enc = LSD iff both are; k = k1 + k2 + 1; l = l1 l2 mod p."""
        al, e, k, l = (C.c_int64 * self.T)(), C.c_int(0), C.c_int64(0), C.c_int64(0)
        _check(lib().lolhip_ct_mul_rule(self._h, int(p), _enc(enc1), int(k1), int(l1), _enc(enc2), int(k2), int(l2), al,
                                        C.byref(e), C.byref(k), C.byref(l)), "ct_mul_rule")
        return al, ("LSD", "MSD")[e.value], int(k.value), int(l.value)

    def ctMul(self, ct1, ct2=None, p=None, cs_crt=False, out_crt=None, stream=None):
        """(*) (SymmSHE.hs:438-452) of ct = (cs, enc, k, l) as ctAdd takes it, any number of components up to 8 each:
        mulG <$> (c1 * c2) with the toLSD factor of the MSD x MSD case folded in (lolhip_ct_mul_batch).  ct2 None, or
        ct1 itself, squares.  cs in the powerful basis, or the CRT basis with cs_crt; the result in the basis out_crt
        asks for (default: that of the inputs).  Returns (cs [na + nb - 1][B][n][T], enc, k, l)."""
        if p is None:
            raise TypeError("ctMul needs the plaintext modulus p")
        square = ct2 is None or ct2 is ct1
        (c1, e1, k1, l1), (c2, e2, k2, l2) = ct1, (ct1 if square else ct2)
        al, enc, k, l = self.ctMulRule(p, e1, k1, l1, e2, k2, l2)
        out_crt = cs_crt if out_crt is None else out_crt
        _, a, na, B = self._cs(c1)
        b, nb = a, na
        if not square:
            _, b, nb, Bb = self._cs(c2)
            if Bb != B:
                raise ValueError("batch sizes differ")
        L = lib()
        out = _run(lambda st, i, o, w, n: L.lolhip_ct_mul_batch(self._h, st, i[0], na, i[0] if square else i[1], nb,
                                                                 int(cs_crt), al, o[0], int(out_crt), w, n),
                   stream, (a,) if square else (a, b), B,
                   lambda: L.lolhip_ct_mul_work_len(self._h, na, nb, int(cs_crt), int(square), B),
                   lambda: (na + nb - 1, B, self.n, self.T))
        return out, enc, k, l

    def _ksCT(self, hint, ct, base, p, cs_crt, stream, deg):
        """toMSD, then c_0 .. c_(deg-1) + switch hint c_deg for a ciphertext of deg + 1 components; a shorter one is
        returned as it is (SymmSHE.hs:343-371)"""
        cs, enc, k, l = ct
        _, cs, ncs, B = self._cs(cs)
        if ncs <= deg:
            return ct
        if ncs > deg + 1:
            raise ValueError(f"a ciphertext of {ncs} components: this key switch takes at most {deg + 1}")
        cs, _, l = self.toMSD(cs, p, enc, l, stream=stream)
        host, (cs, hint) = _stage(cs, hint)
        cs = cs.reshape(ncs, B, self.n, self.T)
        last = cs[deg].clone()
        add = _alloc((2, B, self.n, self.T), "int64", cs.device).zero_()
        add[:deg] = cs[:deg]
        if cs_crt:
            self.crtInv(last, stream=stream)                      # switch decomposes in the powerful basis
        else:
            self.crt(add[:deg], stream=stream)
        return _unstage(host, self.keySwitch(last, base, hint, addend=add, stream=stream)), "MSD", int(k), l

    def keySwitchLinear(self, hint, ct, base, p, cs_crt=False, stream=None):
        """keySwitchLinear (SymmSHE.hs:339-348): toMSD, then (c0 + switch hint c1) for a linear ciphertext
        ct = (cs, enc, k, l) -> (cs [2][B][n][T] in the CRT basis, "MSD", k, l'), a ciphertext under the hint's output
        key; one of fewer components is returned unchanged.  hint: Plan.ksLinearHint's, over the gadget of `base`."""
        return self._ksCT(hint, ct, base, p, cs_crt, stream, 1)

    def keySwitchQuadCirc(self, hint, ct, base, p, cs_crt=False, stream=None):
        """keySwitchQuadCirc (SymmSHE.hs:361-371): toMSD, then ((c0, c1) + switch hint c2) for a quadratic ciphertext
        ct = (cs, enc, k, l) -> (cs [2][B][n][T] in the CRT basis, "MSD", k, l'); one of fewer components is returned
        unchanged.  hint: Plan.ksQuadCircHint's, over the gadget of `base`."""
        return self._ksCT(hint, ct, base, p, cs_crt, stream, 2)

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
        return self.mulPublic(d.reshape(-1), cs, pp.qs[0], stride=0, stream=stream), 0


def mulC(a, b, stream=None):
    """a * b elementwise over complex128 (mulC, types.h:146-152: each product and each sum rounded on its own): with
    crtC / crtInvC the reference's product for moduli without a CRT basis (UCyc CRTExt).  numpy in -> numpy out; a torch
    CUDA tensor a is overwritten.  b may be a."""
    # in place, so not _run; each operand is staged on its own, a numpy b beside a CUDA a being allowed
    host, (ta,) = _stage((a, "complex128"))
    tb = ta if b is a else _stage((b, "complex128"))[1][0]
    pa, pb = _ptr(ta, "complex128"), _ptr(tb, "complex128")
    if ta.numel() != tb.numel():
        raise ValueError("operand sizes differ")
    _check(lib().lolhip_mulc_batch(_stream(stream), pa, pb, ta.numel()), "mulc")
    return _unstage(host, ta)


def chacha20_block(key, counter, nonce):
    """The ChaCha20 block function the samplers run (RFC 8439 §2.3), on the host: 16 uint32 words."""
    nn = (C.c_uint32 * 3)(*[int(x) & 0xFFFFFFFF for x in nonce])
    out = (C.c_uint32 * 16)()
    lib().lolhip_chacha20_block(_key(bytes(key)), int(counter) & 0xFFFFFFFF, nn, out)
    return np.array(list(out), dtype=np.uint32)


class Ext(_Handle):
    """Index tables and kernels for a ring extension m | m' (Tensor.hs:390-509, Extension.hs:54-129)."""
    _kind = "ext"

    def __init__(self, lo: Plan, hi: Plan):
        self.lo, self.hi = lo, hi
        self._create("ext_create", lo._h, hi._h)

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

    def _map(self, op, name, x, to_hi, out, stream, rel=()):
        """one map between the rings, [B] items of src -> rel + [B] items of dst: numpy through lolhip_ext_host, CUDA
        tensors through the batched entry, into `out` when the caller has one"""
        src, dst = (self.lo, self.hi) if to_hi else (self.hi, self.lo)
        B = src._batch(x)
        shape = (*rel, B, dst.n, dst.T)
        if isinstance(x, np.ndarray):
            res = np.zeros(shape, dtype=np.int64)
            _check(lib().lolhip_ext_host(self._h, op, res.ctypes.data_as(_i64p), _np(x)[1], B))
            return res
        if out is None:
            out = _alloc(shape, "int64", x.device)
        _check(getattr(lib(), f"lolhip_{name}_batch")(self._h, _stream(stream), _devptr(out), _devptr(x), B))
        return out

    def coeffs(self, x, out=None, stream=None):
        """[n'/n][B][n][T] coefficient vectors over the relative powerful/decoding basis (Tensor.hs:174)."""
        return self._map(EXT_COEFFS, "coeffs", x, False, out, stream, rel=(self.hi.n // self.lo.n,))

    # evalLin and tunnel make no dry run (dry=False), for the reason given at Plan.ctMulCRT.
    def evalLin(self, es: "Ext", r_dec, ys_crt, stream=None):
        """sum_i ys_i * embed(coeffsDec_i r)  (Linear.hs:75-79): self = E in R, es = E in S;
        r_dec [B][n_R][T] decoding basis, ys_crt [n_R/n_E][n_S][T] CRT basis -> [B][n_S][T] CRT basis."""
        L, B, rel, S = lib(), self.hi._batch(r_dec), self.hi.n // self.lo.n, es.hi
        return _run(lambda st, i, o, w, b: L.lolhip_evallin_batch(self._h, es._h, st, i[0], i[1], o[0], w, b), stream,
                    (r_dec, ys_crt), B, lambda: rel * B * (self.lo.n + S.n) * S.T,      # the coefficients and their embeddings
                    lambda: (B, S.n, S.T), dry=False)

    def tunnel(self, es: "Ext", c0_dec, c1_pow, ys_crt, hints, base, stream=None):
        """SymmSHE `tunnel` after toMSD . absorbGFactors (SymmSHE.hs:549-570): self = E' in R', es = E' in S';
        [c0 (decoding basis), c1 (powerful basis)] over R' -> [2][B][n_S][T] CRT-basis linear ciphertext over S'.
        hints [n_R/n_E][L][2][n_S][T]."""
        L, B, S = lib(), self.hi._batch(c0_dec), es.hi
        return _run(lambda st, i, o, w, b: L.lolhip_tunnel_batch(self._h, es._h, st, i[0], i[1], i[2], i[3], int(base), o[0], w, b),
                    stream, (c0_dec, c1_pow, ys_crt, hints), B, lambda: L.lolhip_tunnel_work_len(self._h, es._h, int(base), B),
                    lambda: (2, B, S.n, S.T), dry=False)

    def tunnelHint(self, es: "Ext", ys_crt, s_in_crt, s_out_crt, svar, base, key=None, ctr=0, stream=None):
        """tunnelHint f skout skin (SymmSHE.hs:531-545): self = E' in R', es = E' in S'; ys_crt [rel][n_S][T] the
        linearDec table of f'q (what tunnel takes), s_in_crt [n_R][T] and s_out_crt [n_S][T] the keys in the CRT bases
        -> hints [rel][L][2][n_S][T] for tunnel.  Uses stream items ctr .. ctr + rel L - 1."""
        L, kb, R, S = lib(), _key(key), self.hi, es.hi
        rel = R.n // self.lo.n
        shapes = [(ys_crt, rel * S.n * S.T), (s_in_crt, R.n * R.T), (s_out_crt, S.n * S.T)]
        if any(_size(a) != want for a, want in shapes):
            raise LolHipError(ERR_INVALID, "tunnelHint: ys_crt, s_in_crt or s_out_crt is not of the plans of the extensions")
        # the entry has no batch and so no dry run: its work_len, asked before anything is staged, raises the host statuses
        wl = _len(L.lolhip_tunnel_hint_work_len(self._h, es._h, int(base)))
        return _run(lambda st, i, o, w, b: L.lolhip_tunnel_hint_batch(self._h, es._h, st, i[0], i[1], i[2], float(svar),
                                                                       int(base), kb, int(ctr), o[0], w),
                    stream, (ys_crt, s_in_crt, s_out_crt), 0, lambda: wl, lambda: (rel, S.decomposeLen(base), 2, S.n, S.T),
                    dry=False)

    def _mapCT(self, ct, maps, basis, what):
        cs, enc, k, l = ct
        if int(k) != 0:
            raise ValueError(f"{what} requires 0 factors of g; call absorbGFactors first")
        if basis not in maps:
            raise ValueError(f"{what}: basis is one of {sorted(maps)}")
        src = self.hi if what == "twaceCT" else self.lo
        _, cs, ncs, B = src._cs(cs)
        out = maps[basis](cs)
        return out.reshape(ncs, B, *out.shape[-2:]), enc, 0, l

    def embedCT(self, ct, basis="pow", stream=None):
        """embedCT (SymmSHE.hs:477-487): embed on every component of ct = (cs, enc, k, l) over the lower ring, cs in
        `basis` ("pow", "dec" or "crt") -> the ciphertext over the higher ring in the same basis.  k must be 0."""
        maps = {"pow": self.embedPow, "dec": self.embedDec, "crt": self.embedCRT}
        return self._mapCT(ct, {b: (lambda x, f=f: f(x, stream=stream)) for b, f in maps.items()}, basis, "embedCT")

    def twaceCT(self, ct, basis="pow", stream=None):
        """twaceCT (SymmSHE.hs:498-503): twace on every component of ct = (cs, enc, k, l) over the higher ring, cs in
        `basis` ("pow", "dec" or "crt") -> the ciphertext over the lower ring in the same basis.  k must be 0."""
        maps = {"pow": self.twacePowDec, "dec": self.twacePowDec, "crt": self.twaceCRT}
        return self._mapCT(ct, {b: (lambda x, f=f: f(x, stream=stream)) for b, f in maps.items()}, basis, "twaceCT")

    def twacePowDec(self, x, out=None, stream=None): return self._map(EXT_TWACE_POWDEC, "twace_powdec", x, False, out, stream)
    def twaceCRT(self, x, out=None, stream=None): return self._map(EXT_TWACE_CRT, "twace_crt", x, False, out, stream)
    def embedPow(self, x, out=None, stream=None): return self._map(EXT_EMBED_POW, "embed_pow", x, True, out, stream)
    def embedDec(self, x, out=None, stream=None): return self._map(EXT_EMBED_DEC, "embed_dec", x, True, out, stream)
    def embedCRT(self, x, out=None, stream=None): return self._map(EXT_EMBED_CRT, "embed_crt", x, True, out, stream)


class TunnelChain(_WorkHandle):
    """tunnelH (HomomPRF.hs:427-431): roundCTUp, the tunnel hops and the roundCTDowns as one call
    (lolhip_tunnel_chain_batch).  exts_er[i] / exts_es[i]: the Exts E'_i in R'_i / E'_i in S'_i of hop i, all over one
    moduli list (the up list); ys[i] [rel_i][n_S][T] and hints[i] [rel_i][L][2][n_S][T]: CUDA tensors as Ext.tunnel
    takes them (kept alive here); p_in / p_out: Plans of the first R' / last S' index over a suffix of the up list."""
    _kind = "tunnel_chain"

    def __init__(self, exts_er, exts_es, ys, hints, base, p_in: Plan, p_out: Plan):
        self.exts_er, self.exts_es, self.ys, self.hint_slabs = list(exts_er), list(exts_es), list(ys), list(hints)
        self.base, self.p_in, self.p_out = int(base), p_in, p_out
        n = len(self.exts_er)
        if not (len(self.exts_es) == len(self.ys) == len(self.hint_slabs) == n):
            raise ValueError("one ext pair, one ys table and one hint slab per hop")
        arr = lambda vals: (C.c_void_p * max(n, 1))(*vals)
        self._create("tunnel_chain_create", n, arr([x._h for x in self.exts_er]), arr([x._h for x in self.exts_es]),
                     arr([_devptr(y) for y in self.ys]), arr([_devptr(x) for x in self.hint_slabs]), self.base, p_in._h,
                     p_out._h)

    def __call__(self, cs, p, enc="LSD", l=1, cs_crt=False, out_crt=False, stream=None):
        """cs [2][B][n_R'][T_in], a linear ciphertext with k = 0 (Plan.absorbGFactors first otherwise), powerful basis or
        CRT basis (cs_crt) -> (out [2][B][n_S'][T_out], "MSD", l')."""
        _, cs, ncs, B = self.p_in._cs(cs)
        if ncs != 2:
            raise LolHipError(ERR_INVALID, "tunnelH takes a linear ciphertext")
        L, lo = lib(), C.c_int64(0)
        args = (int(cs_crt), _enc(enc), int(l), int(p))
        out = _run(
            lambda st, i, o, w, b: L.lolhip_tunnel_chain_batch(self._h, st, i[0], *args, o[0], int(out_crt), C.byref(lo), w, b),
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
        kb = _key(key)
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


class PTTunnel(_WorkHandle):
    """ptTunnel (HomomPRF.hs:510-531): evalLin f_h hop by hop on plaintexts over Z_(p^e) as one call
    (lolhip_pt_tunnel_batch).  exts_er[h] / exts_es[h]: the Exts E_h in R_h / E_h in S_h over ONE NTT prime Q_h per hop
    that exceeds PTTunnel.modulus (certified at creation); funcs[h] [rel_h][n_S_h]: the values of f_h on the relative
    decoding basis, residues mod p^e in the powerful basis (TunnelChain.funcs; numpy or CUDA tensors)."""
    _kind = "pt_tunnel"

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
        self._create("pt_tunnel_create", n, arr([x._h for x in self.exts_er]), arr([x._h for x in self.exts_es]), fp,
                     self.p, self.e)

    @staticmethod
    def modulus(pps_r, pps_s, rel, first_hop, p, e):
        """The exactness bound of one hop (include/lolhip.h): the hop's prime Q must exceed the returned value."""
        (_, a, na), (_, b, nb) = _pps(pps_r), _pps(pps_s)
        return int(_len(lib().lolhip_pt_tunnel_modulus(a, na, b, nb, int(rel), int(bool(first_hop)), int(p), int(e)),
                        "pt_tunnel_modulus"))

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

    def __call__(self, x_dec, stream=None):
        """x_dec [B][n_R0]: plaintexts mod p^e in the decoding basis of R_0 (numpy or a CUDA tensor) -> [B][n_S] residues
        in [0, p^e), powerful basis of the last ring."""
        L = lib()
        call = lambda st, i, o, w, b: L.lolhip_pt_tunnel_batch(self._h, st, i[0], o[0], w, b)
        _dry(call)                                                   # before the shape check
        B = _count(x_dec, self.exts_er[0].hi.n, "x_dec is not a whole number of plaintexts of R_0")
        # min_work=2: this entry carves its work buffer in 16-byte units of two words
        return _run(call, stream, (x_dec,), B, lambda: self.workLen(B), lambda: (B, self.exts_es[-1].hi.n), dry=False,
                    min_work=2)


class RingMul(_WorkHandle):
    """The exact ring product a * b in R_q for moduli without a CRT basis (lolhip_ringmul_batch): q = 2^e, p^e, odd
    composites, tuples of them.  plan_q: any Plan over the moduli; plan_Q: a Plan of the same index over K <= 3 distinct
    NTT primes whose product exceeds 2 C_m floor(q/2)^2 (certified at creation), or None for the primes of
    RingMul.moduli.  Operands and results [B][n][T], powerful basis, numpy or CUDA tensors; operands may be any int64
    (taken mod q_t), results lie in [0, q_t)."""
    _kind = "ringmul"

    def __init__(self, plan_q, plan_Q=None, dense_zq=None, scan_zq=None):
        """dense_zq, scan_zq: passed to the plan_Q made here (None: what plan_q has)"""
        if plan_Q is None:
            plan_Q = Plan(plan_q.pps, self.moduli(plan_q.pps, plan_q.qs), host_only=plan_q.host_only,
                          dense_zq=plan_q.dense_zq if dense_zq is None else dense_zq,
                          scan_zq=plan_q.scan_zq if scan_zq is None else scan_zq)
        self.plan_q, self.plan_Q = plan_q, plan_Q
        self.n, self.T, self.K = plan_q.n, plan_q.T, plan_Q.T
        self._create("ringmul_create", plan_q._h, plan_Q._h)

    @staticmethod
    def moduli(pps, qs):
        """The default NTT primes for index `pps` (a prime-power list or m) and moduli qs: the fewest K <= 3 consecutive
        primes = 1 mod m above the K-th root of 2 C_m floor(max q / 2)^2 (the rule of include/lolhip.h)."""
        _, a, na = _pps(pps)
        qa = (C.c_int64 * max(1, len(qs)))(*[int(q) for q in qs])
        Qs = (C.c_int64 * 3)()
        K = _len(lib().lolhip_ringmul_moduli(a, na, qa, len(qs), Qs), "ringmul_moduli")
        return [int(Qs[i]) for i in range(K)]

    def _batch(self, a):
        return _count(a, self.n * self.T, f"not a whole number of [n={self.n}, T={self.T}] ring elements")

    def __call__(self, a, b, out=None, stream=None):
        """out = a * b; out may be a or b (CUDA tensors), and a may be b."""
        L, B = lib(), self._batch(a)
        if self._batch(b) != B:
            raise ValueError("a and b hold different batches")
        same = b is a
        call = lambda s, i, o, w, n: L.lolhip_ringmul_batch(self._h, s, o[0], i[0], i[0] if same else i[1], w, n)
        return _run(call, stream, [a] if same else [a, b], B, lambda: self.workLen(B), lambda: (B, self.n, self.T), out=out)

    def prepare(self, b, stream=None):
        """bhat [Bb T][n][K]: the CRT over plan_Q of the lifted b [Bb][n][T], for mulPrepared."""
        L, Bb = lib(), self._batch(b)
        call = lambda s, i, o, w, n: L.lolhip_ringmul_prepare(self._h, s, o[0], i[0], w, n)
        return _run(call, stream, [b], Bb, lambda: 0, lambda: (Bb * self.T, self.n, self.K))

    def mulPrepared(self, a, bhat, out=None, stream=None):
        """out = a * b for bhat = prepare(b) of one element (against every item of a) or of as many as a holds."""
        L, B = lib(), self._batch(a)
        Bb = _count(bhat, self.T * self.n * self.K, "bhat is not a whole number of prepared elements")
        call = lambda s, i, o, w, n: L.lolhip_ringmul_prepared_batch(self._h, s, o[0], i[0], i[1], Bb, w, n)
        return _run(call, stream, [a, bhat], B, lambda: self.workLen(B), lambda: (B, self.n, self.T), out=out)


class PTRound(_WorkHandle):
    """ptRound (HomomPRF.hs:215-270): homomorphic rounding from plaintext modulus p = 2^e to 2 as one call
    (lolhip_ptround_batch).  plans[i], i < e: the Plan of index m' over Z_i, each list the one before without its first
    modulus; up_plans[i], i < e - 1: the Plan over U_i = one more modulus in front of Z_i; hints[i] [L_i][2][n'][T(U_i)]:
    ksQuadCircHint of the key over U_i as CUDA tensors (kept alive here; PTRound.hints makes them); pp_m: the Plan of
    index m over p alone (made here when None); exts: (Ext from (m, Z_0) to plans[0], Ext from (m, Z_1) to plans[1]), or
    None for m = m'."""
    _kind = "ptround"

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
        self._create("ptround_create", e, self.p, arr([q._h for q in self.plans]), arr([q._h for q in self.up_plans]),
                     arr([_devptr(x) for x in self.hint_slabs]), self.base, None if pp_m is None else pp_m._h, xs[0],
                     xs[1] if e > 1 else None)

    def __call__(self, cs, enc="MSD", k=0, l=1, cs_crt=False, out_crt=False, stream=None):
        """cs [2][B][n'][T(Z_0)]: CT enc k l over plaintext modulus p, powerful basis or CRT basis (cs_crt) ->
        (out [2][B][n'][T(Z_{e-1})], "MSD", k_out, l_out) over plaintext modulus 2; for e = 1 the input itself, its
        encoding, k and l unchanged."""
        _, cs, ncs, B = self.plans[0]._cs(cs)
        if ncs != 2:
            raise LolHipError(ERR_INVALID, "ptRound takes a linear ciphertext")
        L, ko, lo, last = lib(), C.c_int64(0), C.c_int64(0), self.plans[-1]
        args = (int(cs_crt), _enc(enc), int(k), int(l))
        out = _run(
            lambda st, i, o, w, b: L.lolhip_ptround_batch(self._h, st, i[0], *args, o[0], int(out_crt), C.byref(ko),
                                                           C.byref(lo), w, b),
            stream, (cs,), B, lambda: self.workLen(B), lambda: (2, B, last.n, last.T))
        return out, ("MSD" if len(self.plans) > 1 else ("LSD", "MSD")[_enc(enc)]), int(ko.value), int(lo.value)

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


class KHPRF(_Handle):
    """A family of the key-homomorphic ring PRF of [BP14] over a one-modulus plan (lolhip_khprf_create): a full binary
    tree (preorder leaf counts) and a0, a1 [L][n] in the CRT basis, L = plan.decomposeLen(base).  On a device plan a0,
    a1 and their crt'd gadget decompositions go to HBM once; a host-only plan answers workLen only."""
    _kind = "khprf"

    def __init__(self, plan: Plan, base, tree, a0, a1):
        self._make(plan, None, base, tree, a0, a1)

    @classmethod
    def lifted(cls, plan_q: Plan, plan_Q: Plan, base, tree, a0_pow, a1_pow):
        """The same PRF over q = 2^k, which has no CRT basis (lolhip_khprf_create_lifted): plan_q mod q, plan_Q of the
        same index over an NTT-friendly prime Q in which every node product is exact (certified here), a0_pow, a1_pow
        [L][n] in the powerful basis.  eval() then returns A_T(x) in the powerful basis mod q, and a key s passed to
        __call__ is in the powerful basis of R_q."""
        self = cls.__new__(cls)
        self._make(plan_q, plan_Q, base, tree, a0_pow, a1_pow)
        return self

    def _make(self, plan, plan_Q, base, tree, a0, a1):
        self.plan, self.plan_Q, self.base = plan, plan_Q, int(base)
        self.tree = [int(c) for c in tree]
        self.L = plan.decomposeLen(base) if plan.T == 1 else 0
        a0 = np.ascontiguousarray(np.asarray(a0, dtype=np.int64).reshape(-1))
        a1 = np.ascontiguousarray(np.asarray(a1, dtype=np.int64).reshape(-1))
        if a0.size != self.L * plan.n or a1.size != self.L * plan.n:
            raise ValueError("a0 and a1 must be [L][n]")
        tr = (C.c_int32 * max(1, len(self.tree)))(*self.tree)
        entry, plans = ("khprf_create", (plan._h,)) if plan_Q is None else ("khprf_create_lifted", (plan._h, plan_Q._h))
        self._create(entry, *plans, self.base, tr, len(self.tree), a0.ctypes.data_as(_i64p), a1.ctypes.data_as(_i64p),
                     what=f"{entry}(tree={self.tree})")
        self.k = self.tree[0]

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
        return _len(lib().lolhip_khprf_work_len(self._h, int(x0), int(B)))

    def _window(self, x0, B):
        if int(x0) + int(B) > (1 << self.k) or int(B) < 0:
            _check(ERR_INVALID, "x0 + B > 2^k")

    def eval(self, x0, B, stream=None):
        """A_T(x) for x = x0 .. x0 + B - 1: a CUDA tensor [B][L][n] in the CRT basis (lolhip_khprf_eval_batch); the
        lifted family: in the powerful basis, residues in [0, q)."""
        L = lib()
        call = lambda st, i, o, w, b: L.lolhip_khprf_eval_batch(self._h, st, int(x0), b, o[0], w)
        _dry(call)                                                   # before the window check
        self._window(x0, B)
        return _run(call, stream, (), int(B), lambda: self.workLen(x0, B), lambda: (int(B), self.L, self.plan.n), dry=False)

    def __call__(self, s, p, x0, B, stream=None):
        """ringPRF s x for x = x0 .. x0 + B - 1 (lolhip_khprf_batch): s [n] or [nkeys][n] in the CRT basis (numpy or a
        CUDA tensor; the lifted family: in the powerful basis of R_q) -> [nkeys][B][L][n] int64 in [0, p), decoding
        basis of R_p ([B][L][n] for a single key s [n])."""
        L = lib()
        single = len(s.shape) == 1
        nkeys = 1 if single else int(s.shape[0])
        call = lambda st, i, o, w, b: L.lolhip_khprf_batch(self._h, st, i[0], nkeys, int(p), int(x0), b, o[0], w)
        _dry(call)                                                   # before the window check and the key's lift
        self._window(x0, B)
        # the result stays a CUDA tensor whatever s is: the key goes to the device here, not in _run
        s = self._key_crt(s, nkeys, stream) if self.plan_Q is not None else _stage(s)[1][0]
        out = _run(call, stream, (s.reshape(nkeys, self.plan.n).contiguous(),), int(B), lambda: self.workLen(x0, B),
                   lambda: (nkeys, int(B), self.L, self.plan.n), dry=False)
        return out[0] if single else out


class LatticePRF(_WorkHandle):
    """A family of the key-homomorphic PRF over standard lattices, eq. (2.3) of [BP14] (latticePRF / latticePRFM;
    lolhip_lprf_create): one modulus q (any 2 <= q < 2^62), gadget `base` (0 = TrivGad), a full binary tree (preorder
    leaf counts, as for KHPRF) and a0, a1 [n][K] over Z_q, K = n * ell, ell the gadget length of (base, q).  Without a
    device the family answers workLen only."""
    _kind = "lprf"

    def __init__(self, q, base, tree, a0, a1):
        self.q, self.base, self.tree = int(q), int(base), [int(c) for c in tree]
        a0 = np.ascontiguousarray(np.asarray(a0, dtype=np.int64))
        a1 = np.ascontiguousarray(np.asarray(a1, dtype=np.int64))
        if a0.ndim != 2 or a0.shape != a1.shape:
            raise ValueError("a0 and a1 must be [n][K]")
        if self.q >= 2 and self.base >= 2:                           # gadlen; anything else is the library's to refuse
            ell, t = 0, self.q
            while t:
                ell, t = ell + 1, t // self.base
            if a0.shape[1] != a0.shape[0] * ell:
                raise ValueError(f"a0 and a1 must be [n][K] with K = n * ell = {a0.shape[0] * ell}")
        elif self.base == 0 and a0.shape[1] != a0.shape[0]:
            raise ValueError("a0 and a1 must be [n][n] under TrivGad")
        tr = (C.c_int32 * max(1, len(self.tree)))(*self.tree)
        self._create("lprf_create", self.q, self.base, int(a0.shape[0]), tr, len(self.tree), a0.ctypes.data_as(_i64p),
                     a1.ctypes.data_as(_i64p), what=f"lprf_create(q={q}, base={base}, tree={self.tree})")
        self.n, self.ell = lib().lolhip_lprf_n(self._h), lib().lolhip_lprf_ell(self._h)
        self.K, self.k = self.n * self.ell, self.tree[0]

    def workLen(self, nkeys, x0, B):
        """int64 words of scratch of eval (nkeys = 0) or of a call with nkeys keys over [x0, x0 + B)"""
        return _len(lib().lolhip_lprf_work_len(self._h, int(nkeys), int(x0), int(B)))

    def eval(self, x0, B, stream=None):
        """A_T(x) for x = x0 .. x0 + B - 1: a CUDA tensor [B][n][K] of residues in [0, q) (lolhip_lprf_eval_batch)"""
        L = lib()
        call = lambda st, i, o, w, b: L.lolhip_lprf_eval_batch(self._h, st, int(x0), b, o[0], w)
        _dry(call)                                                   # before the window check
        _len(L.lolhip_lprf_work_len(self._h, 0, int(x0), int(B)), "x0 + B > 2^k")
        return _run(call, stream, (), int(B), lambda: self.workLen(0, x0, B), lambda: (int(B), self.n, self.K), dry=False)

    def __call__(self, s, p, x0, B, stream=None):
        """latticePRF s x for x = x0 .. x0 + B - 1 (lolhip_lprf_batch): s [n] or [nkeys][n], any int64 (numpy or a CUDA
        tensor) -> a CUDA tensor [nkeys][B][K] in [0, p) ([B][K] for a single key s [n]); outputs are indexed by x."""
        L = lib()
        single = len(s.shape) == 1
        nkeys = 1 if single else int(s.shape[0])
        call = lambda st, i, o, w, b: L.lolhip_lprf_batch(self._h, st, i[0], nkeys, int(p), int(x0), b, o[0], w)
        _dry(call)                                                   # before the window check
        _len(L.lolhip_lprf_work_len(self._h, nkeys, int(x0), int(B)), "x0 + B > 2^k")
        s = _stage(s)[1][0]                                          # the result stays a CUDA tensor whatever s is
        out = _run(call, stream, (s.reshape(nkeys, self.n).contiguous(),), int(B), lambda: self.workLen(nkeys, x0, B),
                   lambda: (nkeys, int(B), self.K), dry=False)
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
    def _batch(self, a):
        return _count(a, self.plan.n * self.plan.T, f"a is not a whole number of [n={self.plan.n}, T={self.plan.T}] polynomials")

    def _work_len(self, kind, B):
        return lambda: lib().lolhip_rlwe_work_len(self.plan._h, kind, int(B))

    # ---- gSqNormDec -------------------------------------------------------------------------------------------------
    def gSqNorm(self, e, stream=None):
        """gSqNormDec (Tensor.hs:147-151) of decoding-basis coefficients [B][n] -> [B]: int64 exact or saturated at
        INT64_MAX (also for a coefficient INT64_MIN), float64 with a fixed summation order."""
        L = lib()
        dt = "float64" if str(e.dtype).replace("torch.", "") == "float64" else "int64"
        fn = L.lolhip_gsqnorm_f64_batch if dt == "float64" else L.lolhip_gsqnorm_batch
        call = lambda st, i, o, w, b: fn(self.plan._h, st, i[0], o[0], b)
        _dry(call)                                                   # before the shape check
        B = _count(e, self.plan.n, "e is not [B][n]")
        return _run(call, stream, ((e, dt),), B, None, lambda: [((B,), dt)], dry=False)[0]

    # ---- samplers: CUDA tensors out whatever the secret is given as ---------------------------------------------------
    def secret(self, key=None, ctr=0, stream=None):
        """a uniform secret [n][T] in the CRT basis (Generate.hs:192-218), item ctr of domain 7"""
        L, P, kb = lib(), self.plan, _key(key)
        call = lambda st, i, o, w, b: L.lolhip_rlwe_secret(P._h, st, kb, int(ctr), o[0])
        # the entry has no batch: its dry run can only pass the null output, which it answers with INVALID once every
        # other host status has passed
        _dry(call, tolerate=(ERR_INVALID,))
        return _run(call, stream, (), 0, None, lambda: (P.n, P.T), dry=False)

    def _sample(self, kind, s_crt, B, svar, p, key, ctr, stream):
        L, P, kb, B = lib(), self.plan, _key(key), int(B)
        call = lambda st, i, o, w, nb: L.lolhip_rlwe_sample_batch(P._h, st, kind, int(p), i[0], float(svar), kb, int(ctr),
                                                                  o[0], o[1], w, nb)
        return tuple(_run(call, stream, (s_crt,), B, self._work_len(kind, B),
                          lambda: [((B, P.n, P.T), "int64"), ((B, P.n, P.T) if kind == self.DISC else (B, P.n),
                                                               "float64" if kind == self.CONT else "int64")], unstage=False))

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
        L, P = lib(), self.plan
        call = lambda st, i, o, w, nb: L.lolhip_rlwe_error_batch(P._h, st, kind, i[0], i[1], i[2], o[0], o[1], w, nb)
        _dry(call)                                                   # before the shape checks
        dt = "float64" if kind == self.CONT else "int64"
        B = self._batch(a)
        if _size(b) != B * P.n * (P.T if kind == self.DISC else 1):
            raise ValueError("a and b are not the same number of samples")
        out = _run(call, stream, (a, (b, dt), s_crt), B, self._work_len(kind, B),
                   lambda: [((B, P.n), dt) if want_e else None, ((B,), dt) if want_norm else None], dry=False)
        out = tuple(t for t in out if t is not None)
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
        L, P = lib(), self.plan
        call = lambda st, i, o, w, b: L.lolhip_rlwr_rounded_prod_batch(P._h, int(p), st, i[0], i[1], o[0], w, b)
        _dry(call)                                                   # before the shape check
        B = self._batch(a)
        return _run(call, stream, (a, s_crt), B, self._work_len(self.RLWR, B), lambda: (B, P.n), dry=False)

    def mismatchRLWR(self, s_crt, a, b, p, stream=None):
        """per sample, the coefficients where b differs from roundedProd s a: int32 [B]"""
        L, P = lib(), self.plan
        call = lambda st, i, o, w, nb: L.lolhip_rlwr_check_batch(P._h, int(p), st, i[0], i[1], i[2], o[0], w, nb)
        _dry(call)                                                   # before the shape checks
        B = self._batch(a)
        if _size(b) != B * P.n:
            raise ValueError("a and b are not the same number of samples")
        return _run(call, stream, (a, b, s_crt), B, self._work_len(self.RLWR, B), lambda: [((B,), "int32")], dry=False)[0]

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

    # ---- whole challenges: I instances of L samples, each under its own secret (lolhip_chall_*) -----------------------
    @staticmethod
    def _kind(kind):
        return {"disc": 0, "cont": 1, "rlwr": 2, 0: 0, 1: 1, 2: 2}[kind]

    def instances(self, kind, I, L, svar=1.0, p=0, key=None, ctr_s=0, ctr=0, stream=None):
        """I instances of L samples of `kind` ("disc", "cont", "rlwr" or 0 / 1 / 2) in one call (Generate.hs:105-218):
        CUDA tensors (s [I][n][T], a [I L][n][T], b) in the DECODING basis, the basis of the wire format; b int64
        [I L][n][T] (Disc), float64 [I L][n] (Cont), int64 [I L][n] in [0, p) (RLWR).  Secret i is secret(key, ctr_s + i)
        and sample (i, l) is the single-secret sample at counter ctr + i L + l, taken to the decoding basis.  Never
        reuse the counters ctr_s .. ctr_s + I - 1 and ctr .. ctr + I L - 1 under one key."""
        Lb, P, kb, kind, I, L = lib(), self.plan, _key(key), self._kind(kind), int(I), int(L)
        call = lambda st, i, o, w, nb: Lb.lolhip_chall_generate_batch(P._h, st, kind, int(p), float(svar), kb, int(ctr_s),
                                                                      int(ctr), nb, L, o[0], o[1], o[2], w)
        B = I * L
        return tuple(_run(call, stream, (), I, lambda: Lb.lolhip_chall_work_len(P._h, kind, I, L),
                          lambda: [((I, P.n, P.T), "int64"), ((B, P.n, P.T), "int64"),
                                   ((B, P.n, P.T) if kind == self.DISC else (B, P.n),
                                    "float64" if kind == self.CONT else "int64")], unstage=False))

    def validInstances(self, kind, s_dec, a_dec, b, bound=0, p=0, stream=None):
        """The verdict on I instances in one call (Verify.hs:346-366), all arrays in the decoding basis as instances()
        returns them; L = the samples of a_dec over the secrets of s_dec.  Returns (fails int32 [I], worst [I]): the
        samples of instance i that fail the strict comparison bound > norm (Disc: bound an int; Cont: a float) or
        mismatch (RLWR), and the largest norm (int64, float64) or mismatch count (int64).  Instance i is valid when
        fails[i] == 0."""
        Lb, P, kind = lib(), self.plan, self._kind(kind)
        # an integer norm is below `bound` exactly when it is below its ceiling; beyond int64 only a saturated norm fails
        bd, bc = (max(-2 ** 63, min(2 ** 63 - 1, math.ceil(bound))), 0.0) if kind == self.DISC else (0, float(bound))
        geom = {}
        call = lambda st, i, o, w, nb: Lb.lolhip_chall_verify_batch(P._h, st, kind, int(p), bd, bc, nb, geom.get("L", 1),
                                                                    i[0], i[1], i[2], o[0], o[1], w)
        _dry(call)                                                   # before the shape checks
        I, B = _count(s_dec, P.n * P.T, "s_dec is not [I][n][T]"), self._batch(a_dec)
        if I < 1 or B < 1 or B % I:
            raise ValueError("a_dec is not a whole number of samples per secret")
        if _size(b) != B * P.n * (P.T if kind == self.DISC else 1):
            raise ValueError("a and b are not the same number of samples")
        geom["L"] = B // I
        dt = "float64" if kind == self.CONT else "int64"
        return tuple(_run(call, stream, (s_dec, a_dec, (b, dt)), I, lambda: Lb.lolhip_chall_work_len(P._h, kind, I, B // I),
                          lambda: [((I,), "int32"), ((I,), dt)], dry=False))

    @staticmethod
    def errorBound(m, svar, eps=2.0 ** -25, kind="cont"):
        """errorBound svar eps over index m (host): kind "cont" (Continuous.hs:74-84) a float, "disc" (Discrete.hs:65-76)
        an int"""
        k = {"disc": 0, "cont": 1, 0: 0, 1: 1}[kind]
        _, arr, npp = _pps(int(m))
        out = C.c_double()
        _check(lib().lolhip_rlwe_error_bound(arr, npp, float(svar), float(eps), k, C.byref(out)))
        return int(out.value) if k == 0 else out.value


class RingRLWE:
    """RLWE / RLWR instances over ONE modulus without a CRT basis (lolhip_rlwe_ring_*): q = 2^k, p^e, 105, 500 ..., most
    of rlwe-challenges' parameter list, where RLWE raises "no CRT basis".  a s is the exact ring product of RingMul
    against a prepared secret.  plan_q: a one-modulus Plan; ring: the RingMul made from it (None: RingMul(plan_q)).  The
    class mirrors RLWE with other bases: a [B][n], the secret [n] and Disc b [B][n] are in the POWERFUL basis; Cont b
    float64 [B][n] and RLWR b int64 [B][n] stay in the decoding basis.  Every call takes the prepared secret shat [n][K]
    (secret() returns it beside s_pow; prepare() makes it from a secret of the caller's).  Streams as for RLWE: never
    reuse (key, ctr + b); advance ctr by B between calls."""

    DISC, CONT, RLWR = RLWE.DISC, RLWE.CONT, RLWE.RLWR
    errorBound = staticmethod(RLWE.errorBound)

    def __init__(self, plan_q: Plan, ring=None):
        self.plan = plan_q
        self.ring = RingMul(plan_q) if ring is None else ring
        self.K = self.ring.K

    # ---- helpers ----------------------------------------------------------------------------------------------------
    def _hp(self):
        return self.ring._h, self.plan._h

    def _batch(self, a):
        return _count(a, self.plan.n, f"a is not a whole number of [n={self.plan.n}] polynomials")

    def _work_len(self, kind, B):
        return lambda: lib().lolhip_rlwe_ring_work_len(*self._hp(), kind, int(B))

    def gSqNorm(self, e, stream=None):
        """gSqNormDec of decoding-basis coefficients [B][n] -> [B] (RLWE.gSqNorm: the plan supplies the index only)"""
        return RLWE(self.plan).gSqNorm(e, stream)

    # ---- the secret ---------------------------------------------------------------------------------------------------
    def secret(self, key=None, ctr=0, stream=None):
        """(s_pow [n], shat [n][K]): a uniform secret in the powerful basis, item ctr of domain 7, and its prepared form"""
        L, P, kb, (h, pq) = lib(), self.plan, _key(key), self._hp()
        call = lambda st, i, o, w, b: L.lolhip_rlwe_ring_secret(h, pq, st, kb, int(ctr), o[0], o[1])
        _dry(call, tolerate=(ERR_INVALID,))                          # no batch: the null outputs answer INVALID last
        return tuple(_run(call, stream, (), 0, None, lambda: [((P.n,), "int64"), ((P.n, self.K), "int64")], dry=False))

    def prepare(self, s_pow, stream=None):
        """shat [n][K] of a secret [n] in the powerful basis, any int64 taken mod q (RingMul.prepare)"""
        out = self.ring.prepare(s_pow, stream=stream)
        return out.reshape(self.plan.n, self.K)

    # ---- samplers: CUDA tensors out whatever the secret is given as ---------------------------------------------------
    def _sample(self, kind, shat, B, svar, p, key, ctr, stream):
        L, P, kb, B, (h, pq) = lib(), self.plan, _key(key), int(B), self._hp()
        call = lambda st, i, o, w, nb: L.lolhip_rlwe_ring_sample_batch(h, pq, st, kind, int(p), i[0], float(svar), kb,
                                                                       int(ctr), o[0], o[1], w, nb)
        return tuple(_run(call, stream, (shat,), B, self._work_len(kind, B),
                          lambda: [((B, P.n), "int64"), ((B, P.n), "float64" if kind == self.CONT else "int64")],
                          unstage=False, min_work=2))

    def sampleDisc(self, shat, B, svar, key=None, ctr=0, stream=None):
        """B discrete samples (a, b = a s + l (errorRounded svar) mod q), both [B][n], powerful basis"""
        return self._sample(self.DISC, shat, B, svar, 0, key, ctr, stream)

    def sampleCont(self, shat, B, svar, key=None, ctr=0, stream=None):
        """B continuous samples: a [B][n] powerful basis, b float64 [B][n] in [0, q), decoding basis"""
        return self._sample(self.CONT, shat, B, svar, 0, key, ctr, stream)

    def sampleRLWR(self, shat, B, p, key=None, ctr=0, stream=None):
        """B RLWR samples: a [B][n] powerful basis, b = roundedProd s a [B][n] in [0, p), decoding basis"""
        return self._sample(self.RLWR, shat, B, 1.0, p, key, ctr, stream)

    # ---- error terms and norms ----------------------------------------------------------------------------------------
    def _error(self, kind, shat, a, b, want_e, want_norm, stream):
        L, P, (h, pq) = lib(), self.plan, self._hp()
        call = lambda st, i, o, w, nb: L.lolhip_rlwe_ring_error_batch(h, pq, st, kind, i[0], i[1], i[2], o[0], o[1], w, nb)
        _dry(call)                                                   # before the shape checks
        dt = "float64" if kind == self.CONT else "int64"
        B = self._batch(a)
        if _size(b) != B * P.n:
            raise ValueError("a and b are not the same number of samples")
        out = _run(call, stream, (a, (b, dt), shat), B, self._work_len(kind, B),
                   lambda: [((B, P.n), dt) if want_e else None, ((B,), dt) if want_norm else None], dry=False, min_work=2)
        out = tuple(t for t in out if t is not None)
        return out if len(out) > 1 else out[0]

    def errorTermDisc(self, shat, a, b, norm=False, stream=None):
        """the centred lift of lInv (b - a s): int64 [B][n], decoding basis; norm=True: (e, norm)"""
        return self._error(self.DISC, shat, a, b, True, norm, stream)

    def errorTermCont(self, shat, a, b, norm=False, stream=None):
        """lift (b - a s) in K/(qR): float64 [B][n]; norm=True: (e, norm)"""
        return self._error(self.CONT, shat, a, b, True, norm, stream)

    def errorGSqNormDisc(self, shat, a, b, stream=None):
        """gSqNorm . errorTerm: int64 [B], saturated; the error slab is not returned"""
        return self._error(self.DISC, shat, a, b, False, True, stream)

    def errorGSqNormCont(self, shat, a, b, stream=None):
        """gSqNorm . errorTerm: float64 [B]"""
        return self._error(self.CONT, shat, a, b, False, True, stream)

    # ---- RLWR ---------------------------------------------------------------------------------------------------------
    def roundedProd(self, shat, a, p, stream=None):
        """roundedProd s a: [B][n] in [0, p), decoding basis"""
        L, P, (h, pq) = lib(), self.plan, self._hp()
        call = lambda st, i, o, w, b: L.lolhip_rlwr_ring_rounded_prod_batch(h, pq, int(p), st, i[0], i[1], o[0], w, b)
        _dry(call)                                                   # before the shape check
        B = self._batch(a)
        return _run(call, stream, (a, shat), B, self._work_len(self.RLWR, B), lambda: (B, P.n), dry=False, min_work=2)

    def mismatchRLWR(self, shat, a, b, p, stream=None):
        """per sample, the coefficients where b differs from roundedProd s a: int32 [B]"""
        L, P, (h, pq) = lib(), self.plan, self._hp()
        call = lambda st, i, o, w, nb: L.lolhip_rlwr_ring_check_batch(h, pq, int(p), st, i[0], i[1], i[2], o[0], w, nb)
        _dry(call)                                                   # before the shape checks
        B = self._batch(a)
        if _size(b) != B * P.n:
            raise ValueError("a and b are not the same number of samples")
        return _run(call, stream, (a, b, shat), B, self._work_len(self.RLWR, B), lambda: [((B,), "int32")], dry=False,
                    min_work=2)[0]

    # ---- whole challenges: I instances of L samples, each under its own secret (lolhip_chall_ring_*) ------------------
    def instances(self, kind, I, L, svar=1.0, p=0, key=None, ctr_s=0, ctr=0, stream=None):
        """RLWE.instances over this class's moduli: CUDA tensors (s [I][n], a [I L][n], b [I L][n]) in the DECODING
        basis, b int64 (Disc, RLWR) or float64 (Cont).  Secret i is the s_pow of secret(key, ctr_s + i) and sample (i, l)
        the single-secret sample at counter ctr + i L + l, taken to the decoding basis with lInv."""
        Lb, P, kb, kind, I, L, (h, pq) = lib(), self.plan, _key(key), RLWE._kind(kind), int(I), int(L), self._hp()
        call = lambda st, i, o, w, nb: Lb.lolhip_chall_ring_generate_batch(h, pq, st, kind, int(p), float(svar), kb, int(ctr_s),
                                                                           int(ctr), nb, L, o[0], o[1], o[2], w)
        B = I * L
        return tuple(_run(call, stream, (), I, lambda: Lb.lolhip_chall_ring_work_len(h, pq, kind, I, L),
                          lambda: [((I, P.n), "int64"), ((B, P.n), "int64"),
                                   ((B, P.n), "float64" if kind == self.CONT else "int64")], unstage=False, min_work=2))

    def validInstances(self, kind, s_dec, a_dec, b, bound=0, p=0, stream=None):
        """RLWE.validInstances over this class's moduli: (fails int32 [I], worst [I]) of I instances given in the
        decoding basis, s_dec [I][n], a_dec [I L][n], b [I L][n]"""
        Lb, P, kind, (h, pq) = lib(), self.plan, RLWE._kind(kind), self._hp()
        bd, bc = (max(-2 ** 63, min(2 ** 63 - 1, math.ceil(bound))), 0.0) if kind == self.DISC else (0, float(bound))
        geom = {}
        call = lambda st, i, o, w, nb: Lb.lolhip_chall_ring_verify_batch(h, pq, st, kind, int(p), bd, bc, nb, geom.get("L", 1),
                                                                         i[0], i[1], i[2], o[0], o[1], w)
        _dry(call)                                                   # before the shape checks
        I, B = _count(s_dec, P.n, "s_dec is not [I][n]"), self._batch(a_dec)
        if I < 1 or B < 1 or B % I:
            raise ValueError("a_dec is not a whole number of samples per secret")
        if _size(b) != B * P.n:
            raise ValueError("a and b are not the same number of samples")
        geom["L"] = B // I
        dt = "float64" if kind == self.CONT else "int64"
        return tuple(_run(call, stream, (s_dec, a_dec, (b, dt)), I,
                          lambda: Lb.lolhip_chall_ring_work_len(h, pq, kind, I, B // I),
                          lambda: [((I,), "int32"), ((I,), dt)], dry=False, min_work=2))

    # ---- instance verification: RLWE's comparisons over this class's norms ----------------------------------------------
    validDisc, validCont, validRLWR = RLWE.validDisc, RLWE.validCont, RLWE.validRLWR
