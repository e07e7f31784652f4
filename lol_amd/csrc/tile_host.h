// lol_amd/csrc/tile_host.h — what the launchers of the LDS-tile stage kernels share (k_gauss_dense, k_cplx_dense:
// floatpath.hip; k_zq_dense: zqdense.hip; k_zq_scan: zqscan.hip) and what the host code that routes their stages
// needs (plan.cpp, capi.cpp).  Host code only: it compiles without a device compiler.
#pragma once
#include <cstdio>

#include "plan.h"

namespace lolhip {

// A stage of the tile kernels runs with lanes along r where the stride fills a wave (consecutive lanes, consecutive
// words); below that the lanes go along the rows of the matrix, or the scan goes across lanes.
inline bool lanes_along_r(const Stage& st) { return st.rts >= 64; }

// The stage word of launch_gauss / launch_cplx (kernels.h): the low 8 bits are the number of stages, above them sit
// two bits per stage, its route.  A program of register stages is therefore its plain count.
constexpr int stage_route(int word, int s) { return (word >> (8 + 2 * s)) & 3; }

// Items (polynomials) of a tile: no more than leave about 512 tiles to a batch of B (at least min_want), in whole
// register tiles of J, as far as the cap_items that fit the launcher's LDS allow; one item where not even one fits.
inline i64 tile_items(i64 B, i64 cap_items, int J, i64 min_want = 1) {
  i64 want = (B + 511) / 512;
  if (want < min_want) want = min_want;
  want = (want + J - 1) / J * J;
  i64 items = want < cap_items ? want : cap_items;
  if (items > J) items = items / J * J;
  if (items > B) items = B;
  return items < 1 ? 1 : items;
}

// The info line of a launch, to stderr: `line` holds its head, `at` characters long, and word(p, room, i) prints what
// stage i adds (as snprintf does, and returns).
template <size_t N, typename Word>
void tile_info(char (&line)[N], int at, int nstages, Word word) {
  for (int i = 0; i < nstages && at > 0 && at < (int)N; ++i) at += word(line + at, N - (size_t)at, i);
  fprintf(stderr, "%s\n", line);
}

}  // namespace lolhip
