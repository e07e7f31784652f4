"""Index sets of the dense Gaussian stage tests (tests/test_gauss_dense.py on the GPU, tests/test_gauss_dense_host.py
on the host, tests/golden/make_golden_gauss_dense.py for the fixture).  Inputs, batch, fixture columns and the error
bound are those of tests/float_stages.py.

DENSE_INDICES: a prime above 13 in every index, so every plan has a dense stage (k_gauss_dense, floatpath.hip):
  17, 23, 29, 179, 257, 797   one stage, lts = 1, rts = 1 (n = p - 1 from 16 to 796: tiles of many items)
  46 = 2 23                   the same behind a trivial 2-power factor
  51 = 3 17, 68 = 4 17        rts = 2, a register stage (p = 3) before the dense one at 51
  289 = 17^2                  e = 2: 17 blocks of one stage
  323 = 17 19                 two dense stages (LDS ping-pong), lts > 1 at the first, rts = 16 at the second
  2^9 17, 2^10 17             rts = 256 / 512: lanes along r; n = 4096 and n = 8192
PARITY_INDICES: every prime at most 13, so both routes exist; under the GAUSS_DENSE switch 7 and 13 run one dense stage,
45 = 9 5 two with rts = 1 and 6, 1456 = 16 7 13 two with rts = 8 and 48, 5600 = 32 25 7 one with lanes along the rows
(rts = 16) and one with lanes along r (rts = 320).
"""
DENSE_INDICES = [17, 23, 29, 179, 257, 797, 46, 51, 68, 289, 323, 2 ** 9 * 17, 2 ** 10 * 17]
PARITY_INDICES = [7, 13, 45, 1456, 5600]
