"""Case table of the persistent pipelined poly-mul k_pow2_pipe<L, AR, SQ> (pow2_pipe.hip): plain data and helpers shared
by test_pipe_host.py (coverage and the integer model, no GPU) and test_pipe.py (the kernel itself).

Moduli     both ends of every 32-bit arithmetic class as pow2_impl.h / plan.cpp number them (q < 2^27: 4, < 2^30: 2,
           < 2^31: 3), all = 1 mod 2^14, so each serves L = 12 and L = 13
Rows       nine operand pairs per modulus: extreme and structured residues whose negacyclic products have closed forms,
           and two random rows.  The stored powerful basis is bit-reversed (position j holds the coefficient of
           X^bitrev(j), pow2_impl.h), which the closed forms below account for
Routes     every (L, modulus, squaring) triple: the twelve instantiations, each at the bottom and the top of its class
Rounds     grid overrides G and batch sizes around them: every workgroup of the persistent loop makes one, two and three
           iterations, some one fewer than others
"""
import numpy as np

from oracle import lolmath as lm
from saturate import class_top

M = 2 ** 14
LS = (12, 13)
CLASS_BOUND = {4: 2 ** 27, 2: 2 ** 30, 3: 2 ** 31}            # exclusive upper bound of each class
TOP = {4: class_top(M, "27")[0], 2: class_top(M, "30")[0], 3: class_top(M, "31")[0]}
BOTTOM = {4: 65537, 2: lm.first_good_q(M, 2 ** 27), 3: 1073872897}
MODULI = [BOTTOM[4], TOP[4], BOTTOM[2], TOP[2], BOTTOM[3], TOP[3]]


def arith_class(q):
    """plan.cpp: the 32-bit arithmetic class of a single odd modulus below 2^31"""
    assert q % 2 == 1 and q < 2 ** 31
    return 4 if q < 2 ** 27 else 2 if q < 2 ** 30 else 3


ROW_NAMES = ("max_max", "negmax_max", "alternating", "zero", "minus_one", "delta0", "wrap", "random", "random_signed")
ROW = {nm: i for i, nm in enumerate(ROW_NAMES)}


def bitrev(L):
    """j -> bitrev_L(j) for j < 2^L"""
    j = np.arange(1 << L, dtype=np.int64)
    r = np.zeros_like(j)
    for k in range(L):
        r |= ((j >> k) & 1) << (L - 1 - k)
    return r


def rows(q, L, seed=0):
    """(a, b): int64 [9][n][1] operand rows in ROW_NAMES order, representatives in (-q, q)"""
    n = 1 << L
    rng = np.random.default_rng([seed, L, q])
    a, b = np.zeros((len(ROW_NAMES), n), dtype=np.int64), np.zeros((len(ROW_NAMES), n), dtype=np.int64)
    a[ROW["max_max"]] = q - 1
    b[ROW["max_max"]] = q - 1
    a[ROW["negmax_max"]] = -(q - 1)
    b[ROW["negmax_max"]] = q - 1
    alt = np.where(np.arange(n) % 2 == 0, q - 1, -(q - 1))     # stored position parity = top bit of the exponent
    a[ROW["alternating"]] = alt
    b[ROW["alternating"]] = -alt
    b[ROW["zero"]] = rng.integers(-(q - 1), q, size=n)
    a[ROW["minus_one"]] = -1
    b[ROW["minus_one"]] = -1
    a[ROW["delta0"], 0] = 1
    b[ROW["delta0"]] = rng.integers(0, q, size=n)
    a[ROW["wrap"], n - 1] = 1                                   # X^(n-1): bitrev(n - 1) = n - 1
    b[ROW["wrap"], n // 2] = 1                                  # X: bitrev(1) = n / 2
    a[ROW["random"]] = rng.integers(0, q, size=n)
    b[ROW["random"]] = rng.integers(0, q, size=n)
    a[ROW["random_signed"]] = rng.integers(-(q - 1), q, size=n)
    b[ROW["random_signed"]] = rng.integers(-(q - 1), q, size=n)
    return a.reshape(-1, n, 1), b.reshape(-1, n, 1)


def closed_forms(q, L, a, b, square=False):
    """{row name: int64 [n] canonical product} for the rows that have one; square: of a * a instead of a * b.
    With J = 1 + X + ... + X^(n-1) and J0 = 1 + ... + X^(n/2-1) in Z_q[X] / (X^n + 1):
      J^2 has coefficient 2k + 2 - n at X^k;   (X^(n/2) - 1)^2 = -2 X^(n/2), and J0^2 has k + 1 below n/2, n - 1 - k from
      n/2 on, so (J0 (X^(n/2) - 1))^2 has 2 (n/2 - 1 - e) at e < n/2 and -2 (e - n/2 + 1) at e >= n/2."""
    n = 1 << L
    e = bitrev(L)                                               # exponent held by each stored position
    jj = 2 * e + 2 - n
    lo = e < n // 2
    alt2 = np.where(lo, 2 * (n // 2 - 1 - e), -2 * (e - n // 2 + 1))
    zero = np.zeros(n, dtype=np.int64)
    out = {}
    out["max_max"] = jj                                         # (-J)(-J)
    out["negmax_max"] = jj if square else -jj                   # J J; J (-J)
    out["alternating"] = alt2 if square else -alt2
    out["zero"] = zero
    out["minus_one"] = jj
    d0 = zero.copy()
    d0[0] = 1
    out["delta0"] = d0 if square else np.mod(b[ROW["delta0"]].reshape(n), q)
    w = zero.copy()
    w[int(np.nonzero(e == n - 2)[0][0]) if square else 0] = -1  # X^(2n-2) = -X^(n-2);  X^(n-1) X = X^n = -1
    out["wrap"] = w
    return {k: np.mod(v, q).astype(np.int64) for k, v in out.items()}


# ---- routes: every instantiation, at the bottom and at the top of its class ----------------------------------------
ROUTE_CASES = [(L, q, sq) for L in LS for q in MODULI for sq in (False, True)]

# ---- round shapes of the persistent loop ---------------------------------------------------------------------------
ROUND_GRIDS = (1, 2, 3, 5)
ROUND_PLANS = [(13, TOP[4]), (13, TOP[2]), (13, TOP[3]), (12, TOP[3])]
ROUND_BMAX = 3 * max(ROUND_GRIDS) - 1


def round_batches(G):
    return sorted({B for B in (1, G - 1, G, G + 1, 2 * G, 2 * G + 1, 3 * G - 1) if B > 0})


# ---- the real grid: two workgroups per CU, so 2048 is four whole rounds of 512 on a 256-CU device --------------------
REAL_L, REAL_Q = 13, TOP[2]
REAL_THRESHOLD = 2048                                           # pow2_pipe_ok: the default route from here up
REAL_FORCED = 2 * 1024 + 1
REAL_ALIAS_B = 1100
