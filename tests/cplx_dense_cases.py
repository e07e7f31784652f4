"""Index sets of the dense complex CRT tests (tests/test_cplx_dense.py on the GPU, tests/test_cplx_dense_host.py on the
host, tests/golden/make_golden_cplx_dense.py for the fixture).  Inputs, batch and fixture columns are those of
tests/float_stages.py; the bound is the float members' contract, 1e-12 max(1, max |expected|).

DENSE_INDICES: a prime above 13 in every index, so every opted-in plan has a dense stage (k_cplx_dense, floatpath.hip):
  17            d = 16: one exact 16 x 16 x 4 tile row, no tails
  19, 23        d = 18, 22: a row tail (two tile rows, the second 2 / 6 rows) and a depth tail (18 = 4 4 + 2)
  68 = 4 17     rts = 2 behind a 2-power stage (and a DIAG stage of its own in front)
  51 = 3 17     a register stage (p = 3) before the dense one
  289 = 17^2    a d = 16 CRT stage with the folded crtTwiddle diagonal, then a d = 17 DFT stage at stride 16: two dense
                stages, LDS ping-pong, both operand orders of the matrix route (stride below / from 16)
  323 = 17 19   two dense stages of different primes, ping-pong, the last one to the slab
  257           a long vector: 16 tile rows, and exactly 16 columns in a full LDS tile
  797           50 tile rows, but an LDS tile holds 5 columns: the route rule keeps this one on the vector ALU
  2^9 17        n = 4096, stride 256: lanes along r on the vector ALU
  2^10 17       n = 8192: one 128 KiB buffer, possible only because the dense stage is the last and writes the slab
PARITY_INDICES: every prime at most 13, so the register route exists; under CPLX_DENSE every odd prime's stages run
dense (the matrix route, or the vector ALU with CPLX_DENSE_VALU as well): 7, 13 one stage; 45 = 9 5 three (d = 2, 3, 4);
1456 = 16 7 13 two at strides 8 and 48; 5600 = 32 25 7 three, strides 16, 64 (lanes along r) and 320.
LARGE_PARITY: indices of DENSE_INDICES whose matrix route (the route rule's own choice) is compared with the vector ALU's;
at 797 it is the other way round: the rule's choice is the vector ALU and CPLX_DENSE puts the stage on the matrix cores.
"""
DENSE_INDICES = [17, 19, 23, 68, 51, 289, 323, 257, 797, 2 ** 9 * 17, 2 ** 10 * 17]
PARITY_INDICES = [7, 13, 45, 1456, 5600]
LARGE_PARITY = [17, 289, 257]


def dense_routes(prog, n):
    """The route rule restated (plan.cpp): for the rows (kind, prime, length, stride, ...) of a program, 0 for a register
    stage or a diagonal, else 2 (matrix cores) where the vector fills a 16-row tile (d >= 16) and the largest LDS tile
    (64 KiB, or one item) holds 16 columns, n / d per item, else 1 (vector ALU).  Dense: DFT_p, CRT_p, CRT_p^-1 of p > 13.
    Two LDS buffers when a dense stage is followed by another stage."""
    rows = [r[:4] for r in prog]
    dense = [k in (1, 2, 3) and p > 13 for k, p, d, rts in rows]
    nbuf = 2 if any(dense[:-1]) else 1
    per = nbuf * 16 * n
    items = 64 * 1024 // per if per < 64 * 1024 else 1
    return [0 if not dn else (2 if d >= 16 and items * (n // d) >= 16 else 1) for dn, (k, p, d, rts) in zip(dense, rows)]
