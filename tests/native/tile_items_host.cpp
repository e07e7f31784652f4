// tests/native/tile_items_host.cpp — the tile picker of the LDS-tile stage kernels (tile_items, tile_host.h) with each
// launcher's cap rule, a stand-alone host program (tests/test_tile_items_host.py builds and runs it).  The expected
// values are the arithmetic the four launchers carried, each its own copy, before they shared the picker: restated below
// as they were written (old_dense: launch_gauss and launch_zq_dense; old_cplx: launch_cplx; old_scan: launch_zq_scan),
// compared over a grid, and worked out by hand for the cases the GPU tests' info lines assert too.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "tile_host.h"

using lolhip::i64;
using lolhip::tile_items;

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

static i64 old_dense(i64 B, i64 cap, i64 J) {
  i64 want = (B + 511) / 512;
  want = (want + J - 1) / J * J;
  i64 items = want < cap ? want : cap;
  if (items > J) items = items / J * J;
  if (items > B) items = B;
  if (items < 1) items = 1;
  return items;
}
static i64 old_cplx(i64 B, i64 cap) {
  i64 items = (B + 511) / 512;
  if (items > cap) items = cap;
  if (items > B) items = B;
  if (items < 1) items = 1;
  return items;
}
static i64 old_scan(i64 B, i64 cap, i64 n) {
  i64 want = (B + 511) / 512;
  if (want < (1024 + n - 1) / n) want = (1024 + n - 1) / n;
  i64 items = want < cap ? want : cap;
  if (items > B) items = B;
  if (items < 1) items = 1;
  return items;
}

// the launchers' caps: bytes of LDS a tile may take over the bytes of one item (every buffer of it)
static i64 cap_gauss(i64 n, int nbuf, bool rows) { return (rows ? 64 : 32) * 1024 / (nbuf * n * 8); }
static i64 cap_cplx(i64 n, int nbuf) { return 64 * 1024 / (nbuf * n * 16); }
static i64 cap_zq(i64 n, i64 word, bool rows_or_mfma, bool polymul) { return (rows_or_mfma ? 64 : 32) * 1024 / ((polymul ? 4 : 2) * n * word); }
// launch_zq_dense on the matrix cores: where 64 KiB hold fewer than 32 columns (cpi = columns per item, n / dmax, twice
// that for the poly-mul), the cap grows towards 32 columns within the 152 KiB budget
static i64 cap_zq_mfma(i64 n, i64 cpi, bool polymul) {
  const i64 per = (polymul ? 4 : 2) * n * 4;
  i64 cap = 64 * 1024 / per;
  if (cap * cpi < 32) { const i64 big = 152 * 1024 / per, full = (32 + cpi - 1) / cpi; cap = big < full ? big : full; }
  return cap;
}
static i64 cap_scan(i64 n, i64 word) { return 64 * 1024 / (n * word); }
static i64 floor_scan(i64 n) { return (1024 + n - 1) / n; }

int main() {
  // gauss, n = 22, one buffer, rows layout: 372 items fit; 5000 / 512 -> 10 -> two register tiles of 8
  CHECK(cap_gauss(22, 1, true) == 372);
  CHECK(tile_items(5000, cap_gauss(22, 1, true), 8) == 16);
  CHECK((5000 + 16 - 1) / 16 == 313);
  // cplx, n = 22, no register tile: ceil(B / 512)
  CHECK(tile_items(1535, cap_cplx(22, 1), 1) == 3);
  CHECK(tile_items(1536, cap_cplx(22, 1), 1) == 3);
  CHECK(tile_items(1537, cap_cplx(22, 1), 1) == 4);
  // cplx, n = 288, two buffers of 4608 B each per item
  CHECK(cap_cplx(288, 2) == 7);
  CHECK(tile_items(100000, cap_cplx(288, 2), 1) == 7);
  // zq dense, n = 8192 at 8-byte words: the ping-pong pair takes 128 KiB, no item fits 64 KiB, the tile is one item
  CHECK(cap_zq(8192, 8, true, false) == 0 && cap_zq(8192, 8, false, false) == 0);
  CHECK(tile_items(100000, 0, 4) == 1);
  // zq dense, the cap cuts to whole register tiles: n = 272 at 4-byte words, rows: 30 items fit, 24 are taken
  CHECK(cap_zq(272, 4, true, false) == 30);
  CHECK(tile_items(100000, 30, 8) == 24);
  CHECK(tile_items(100000, 7, 8) == 7);                    // below one register tile the cap stands
  // zq dense on the matrix cores, m = 797 (n = 796, one column per item): 10 items fit 64 KiB, the cap grows to the 24
  // the budget holds (32 asked for); m = 257 (n = 256): 32 items fit as they are; the poly-mul at 797: 12 of 16 asked for
  CHECK(cap_zq_mfma(796, 1, false) == 24 && tile_items(5269, 24, 32) == 24);
  CHECK(cap_zq_mfma(256, 1, false) == 32 && tile_items(16384, 32, 32) == 32);
  CHECK(cap_zq_mfma(796, 2, true) == 12 && tile_items(5269, 12, 32) == 12);
  // scan, n = 8192 at 8-byte words: one item of exactly 64 KiB
  CHECK(cap_scan(8192, 8) == 1);
  CHECK(tile_items(100000, cap_scan(8192, 8), 1, floor_scan(8192)) == 1);
  // scan, n = 16: the 1024-word floor gives 64 items where B / 512 asks for 2
  CHECK(floor_scan(16) == 64 && cap_scan(16, 4) == 1024);
  CHECK(tile_items(1000, cap_scan(16, 4), 1, floor_scan(16)) == 64);
  CHECK(tile_items(1000, cap_scan(16, 8), 1, floor_scan(16)) == 64);
  CHECK(tile_items(40, cap_scan(16, 4), 1, floor_scan(16)) == 40);      // never more than the batch
  // B below the register tile: items = B; B = 1: one item; every family
  for (i64 B = 1; B < 8; ++B) {
    CHECK(tile_items(B, cap_gauss(22, 1, true), 8) == B);
    CHECK(tile_items(B, cap_gauss(22, 2, false), 8) == B);
    CHECK(tile_items(B, cap_zq(272, 4, true, false), 8) == B);
    if (B < 4) CHECK(tile_items(B, cap_zq(272, 8, false, true), 4) == B);
    CHECK(tile_items(B, cap_zq(16, 4, true, false), 32) == B);          // the matrix cores' 32-column tile
  }
  CHECK(tile_items(1, cap_cplx(22, 1), 1) == 1);
  CHECK(tile_items(1, cap_scan(16, 4), 1, floor_scan(16)) == 1);
  CHECK(tile_items(1, 0, 8) == 1);
  // the grid: every register tile, caps around them, batches around the multiples of 512
  long cases = 0;
  const i64 Bs[] = {1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 37, 511, 512, 513, 1535, 1536, 1537, 4095, 4096, 4097, 5000, 16384, 100000, 1 << 20};
  for (i64 B : Bs)
    for (i64 cap = 0; cap <= 1100; cap += (cap < 70 ? 1 : 103)) {
      for (i64 J : {4, 8, 32}) { CHECK(tile_items(B, cap, (int)J) == old_dense(B, cap, J)); ++cases; }
      CHECK(tile_items(B, cap, 1) == old_cplx(B, cap)); ++cases;
      for (i64 n : {1, 16, 22, 256, 1023, 1024, 1025, 8192}) { CHECK(tile_items(B, cap, 1, floor_scan(n)) == old_scan(B, cap, n)); ++cases; }
    }
  std::printf("tile items host ok: %ld cases\n", cases);
  return 0;
}
