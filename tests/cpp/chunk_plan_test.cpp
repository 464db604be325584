// chunk_plan (etcd_amd/csrc/qe_launch.hpp) against values worked by hand from
// the five launch sites it replaced: launch_cv_stream and launch_repl_stream
// (an override is taken as given), launch_progress_send, launch_check_quorum
// and qe_confchange (an override is floored at 2 as the automatic chunk is).
// Host only: no GPU, no library.  And tile_grid, the grid of the kernels that
// give each wave one tile (the four dispatchers of qe_tick and the step kernels
// it replaced): a block per 4 tiles, at least 1, with statistics at most 8 per
// CU.
//
// The rule, for `tiles` 64-group tiles, 256 CUs and at most 8 tiles per wave:
//   automatic chunk = max(2, ceil(tiles / (256 * 32))), then min(8, .);
//   blocks = ceil(tiles / (4 waves * chunk)); more than 2^31 - 1: QE_ERANGE.
#include <stdio.h>

#include "../../etcd_amd/csrc/qe_launch.hpp"

static int failures = 0;

static void expect(const char *what, uint64_t tiles, int over, bool floor_over, int status,
                   uint32_t chunk, uint32_t blocks) {
  const qe::ChunkPlan p = qe::chunk_plan(tiles, 256, over, 8, floor_over);
  const bool ok = p.status == status && (status != QE_OK || (p.chunk == chunk && p.blocks == blocks));
  if (!ok) {
    failures++;
    printf("FAIL %s: tiles %llu override %d floor %d -> status %d chunk %u blocks %u, want %d %u %u\n",
           what, static_cast<unsigned long long>(tiles), over, floor_over ? 1 : 0, p.status, p.chunk,
           p.blocks, status, chunk, blocks);
  }
}

static void expect_grid(const char *what, uint64_t groups, bool stats, uint32_t blocks) {
  const uint32_t got = qe::tile_grid(groups, 256, stats);
  if (got != blocks) {
    failures++;
    printf("FAIL %s: groups %llu stats %d -> %u blocks, want %u\n", what,
           static_cast<unsigned long long>(groups), stats ? 1 : 0, got, blocks);
  }
}

// 256 CUs: the cap is 2048 blocks = 8192 tiles = 524288 groups
static void tile_grid_cases() {
  for (int st = 0; st < 2; st++) {
    const bool s = st != 0;
    expect_grid("no group", 0, s, 1);
    expect_grid("one group", 1, s, 1);
    expect_grid("one block of tiles", 4 * 64, s, 1);
    expect_grid("one group more", 4 * 64 + 1, s, 2);
    expect_grid("one tile more", 5 * 64, s, 2);
    expect_grid("the cap", 2048ull * 4 * 64, s, 2048);
  }
  expect_grid("the cap plus one group, statistics", 2048ull * 4 * 64 + 1, true, 2048);
  expect_grid("the cap plus one group", 2048ull * 4 * 64 + 1, false, 2049);
  expect_grid("the walking-wave tests' batch, statistics", (2 * 8192 + 2) * 64ull + 21, true, 2048);
  expect_grid("the same without", (2 * 8192 + 2) * 64ull + 21, false, 4097);
  // 2^31 - 1 blocks hold every batch of fewer than 2^39 groups
  expect_grid("largest grid", 0x7FFFFFFFull * 256, false, 0x7FFFFFFFu);
  expect_grid("past it", 0x7FFFFFFFull * 256 + 1, false, 0x7FFFFFFFu);
}

int main() {
  tile_grid_cases();
  for (int fl = 0; fl < 2; fl++) {
    const bool f = fl != 0;
    // automatic chunk (override -1, and 0 = "persistent grid", which the
    // chunked kernels treat as automatic): the floor flag does not matter
    for (int over = -1; over <= 0; over++) {
      expect("one tile", 1, over, f, QE_OK, 2, 1);
      expect("two tiles", 2, over, f, QE_OK, 2, 1);
      expect("last automatic chunk of 1", 8192, over, f, QE_OK, 2, 1024);  // 8192 / 8
      expect("first automatic chunk of 2", 8193, over, f, QE_OK, 2, 1025); // ceil(8193 / 8)
      expect("chunk 9 clamped", 65537, over, f, QE_OK, 8, 2049);          // ceil(65537 / 32)
      expect("16M groups", 262144, over, f, QE_OK, 8, 8192);              // chunk 32 -> 8
    }
    // overrides on 1000 tiles: 2, 8 and 9 (clamped to 8) do not see the floor
    expect("override 2", 1000, 2, f, QE_OK, 2, 125);
    expect("override 8", 1000, 8, f, QE_OK, 8, 32);  // ceil(1000 / 32)
    expect("override 9", 1000, 9, f, QE_OK, 8, 32);
    // the grid limit, at chunk 8 (32 tiles per block)
    const uint64_t edge = 32ull * 0x7FFFFFFFull;
    expect("largest grid", edge, -1, f, QE_OK, 8, 0x7FFFFFFFu);
    expect("grid too large", edge + 1, -1, f, QE_ERANGE, 0, 0);
    expect("grid too large, override", edge + 1, 8, f, QE_ERANGE, 0, 0);
  }
  // override 1: a chunk of 1 for the stream kernels, floored for the others
  expect("override 1, stream", 1000, 1, false, QE_OK, 1, 250);
  expect("override 1, floored", 1000, 1, true, QE_OK, 2, 125);
  expect("override 1, stream, one tile", 1, 1, false, QE_OK, 1, 1);
  // a chunk of 1 reaches the grid limit at 4 tiles per block
  expect("override 1, stream, grid too large", 4ull * 0x7FFFFFFFull + 1, 1, false, QE_ERANGE, 0, 0);
  expect("override 1, floored, same tiles", 4ull * 0x7FFFFFFFull + 1, 1, true, QE_OK, 2, 0x40000000u);
  if (failures) return 1;
  printf("PASS: chunk plan\n");
  return 0;
}
