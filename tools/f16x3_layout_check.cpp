// Stand-alone CPU check of the index functions of csrc/f16x3_tile.h, the ones the f16x3 kernels themselves call: build it with a host
// compiler and -fsanitize=address,undefined and run it; it needs no GPU and no HIP.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I unitspeech_amd/csrc tools/f16x3_layout_check.cpp -o /tmp/f16x3_check && /tmp/f16x3_check
//
// Chunk image (conv_igemm_kernel, wino_persist_kernel) and stream image (wino_stream_kernel, K = 128 and 256): the DMA's source-side map
// fills every 16-byte slot once, with the piece the fragment reads expect there, and the 16 lanes of every ds_read_b128 lane group hit
// 16 distinct slots of the 256-byte bank window.  Turn-round patch: every (row, column) is written once and read once, inside the
// patch.  mfma32_row is a bijection onto 0..31.
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "f16x3_tile.h"

using namespace us;

static int failures = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAILED %s (line %d)\n", #c, __LINE__);               \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

// the four 16-lane groups that one ds_read_b128 is serviced in (one LDS cycle each when conflict-free)
static const int kLaneGroups[4][16] = {
    {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
    {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
    {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63},
};

// 16-byte slot indices (one per lane) -> all 16 lanes of every group in distinct slots of the 256-byte window
static void check_banks(const int (&slot)[64]) {
  for (const auto& g : kLaneGroups) {
    std::set<int> w;
    for (int l : g) w.insert(slot[l] % 16);
    CHECK(w.size() == 16);
  }
}

// Chunk image of `rows` rows x bk channels: a wave-wide piece covers 64 / (bk / 4) rows, lane l feeds (row lane / cpr, slot lane % cpr).
static void check_chunk_image(int bk, int rows) {
  const int cpr = bk / 4, rpi = 64 / cpr;
  std::vector<int> image(rows * cpr, -1);             // slot -> source piece of its row
  for (int piece = 0; piece < rows / rpi; ++piece)
    for (int lane = 0; lane < 64; ++lane) {
      const int r = piece * rpi + lane / cpr, pos = lane % cpr;
      const int src = chunk_slot(r, pos, bk);
      CHECK(src >= 0 && src < cpr && image[r * cpr + pos] == -1);
      image[r * cpr + pos] = src;
    }
  for (int v : image) CHECK(v >= 0);
  for (int r = 0; r < rows; ++r) {
    std::set<int> seen(image.begin() + r * cpr, image.begin() + (r + 1) * cpr);
    CHECK((int)seen.size() == cpr);                   // every piece of the row is somewhere in the row
  }
  // the reads: block i of a wave's rows starts 32 i rows further, lane l reads row base + (l & 31)
  for (int base = 0; base + 32 <= rows; base += 32) {
    CHECK(chunk_swz(base + 5, bk) == chunk_swz(5, bk));      // the swizzle of a lane's row is the same in every block
    if (bk == 32) {
      for (int s = 0; s < 2; ++s)
        for (int p = 0; p < 2; ++p) {
          int slot[64];
          for (int lane = 0; lane < 64; ++lane) {
            const int r = base + (lane & 31), want = f16x3_piece(s, lane >> 5, p);
            slot[lane] = r * cpr + chunk_slot(r, want, bk);
            CHECK(image[slot[lane]] == want);         // plane p of channels 16 s + 8 hh .. + 7
          }
          check_banks(slot);
        }
    }
    for (int s = 0; s < bk / 8; ++s) {                // the fp32 form: piece 2 s + hh is channels 8 s + 4 hh .. + 3
      int slot[64];
      for (int lane = 0; lane < 64; ++lane) {
        const int r = base + (lane & 31), want = 2 * s + (lane >> 5);
        slot[lane] = r * cpr + chunk_slot(r, want, bk);
        CHECK(image[slot[lane]] == want);
      }
      check_banks(slot);
    }
  }
  std::set<int> pieces;                                // the F16 reads of a chunk take every piece of a row once
  for (int s = 0; s < 2; ++s)
    for (int hh = 0; hh < 2; ++hh)
      for (int p = 0; p < 2; ++p) pieces.insert(f16x3_piece(s, hh, p));
  CHECK(pieces.size() == 8 && *pieces.begin() == 0 && *pieces.rbegin() == 7);
}

// Stream image: a 32-row tile, K / 4 slots per row; wave w, piece j, lane l feeds slot 64 (w P + j) + l, P = K / 64
static void check_stream_image(int K) {
  const int cprk = K / 4, P = K / 64;
  std::vector<std::pair<int, int>> image(32 * cprk, {-1, -1});
  for (int wave = 0; wave < 8; ++wave)
    for (int j = 0; j < P; ++j)
      for (int lane = 0; lane < 64; ++lane) {
        const int slot = (wave * P + j) * 64 + lane;
        const int r = slot / cprk, pos = slot % cprk;
        CHECK(slot < 32 * cprk && image[slot].first == -1);
        const int src = stream_slot(r, pos);
        CHECK(src >= 0 && src < cprk);
        image[slot] = {r, src};
      }
  for (const auto& e : image) CHECK(e.first >= 0);
  for (int s = 0; s < K / 16; ++s)
    for (int p = 0; p < 2; ++p) {
      int slot[64];
      for (int lane = 0; lane < 64; ++lane) {
        const int r = lane & 31, want = f16x3_piece(s, lane >> 5, p);
        slot[lane] = r * cprk + stream_slot(r, want);
        CHECK(slot[lane] < 32 * cprk && image[slot[lane]] == std::make_pair(r, want));
      }
      check_banks(slot);
    }
}

static void check_turn_round() {
  std::vector<int> written(kTurnFloats, 0), read(kTurnFloats, 0);
  std::set<std::pair<int, int>> cells;
  for (int lane = 0; lane < 64; ++lane)
    for (int r = 0; r < 16; ++r) {
      const int at = turn_write_at(r, lane);
      CHECK(at >= 0 && at < kTurnFloats);
      CHECK(at == turn_write_at(0, lane) + mfma32_row(r, 0) * kTurnLd);      // turn_round writes through one base pointer per lane
      CHECK(at == mfma32_row(r, lane >> 5) * kTurnLd + (lane & 31));         // row of the block, column of the block
      ++written[at];
      cells.insert({at / kTurnLd, at % kTurnLd});
    }
  CHECK(cells.size() == 32 * 32);
  for (int lane = 0; lane < 64; ++lane)
    for (int k = 0; k < 4; ++k) {
      const int row = turn_read_row(k, lane), col = turn_read_col(lane);
      CHECK(row >= 0 && row < 32 && col >= 0 && col + 3 < 32 && (row * kTurnLd + col) % 4 == 0);      // a 16-byte read inside the row
      CHECK(row == turn_read_row(0, lane) + 8 * k);
      for (int q = 0; q < 4; ++q) ++read[row * kTurnLd + col + q];
    }
  for (int row = 0; row < 32; ++row)
    for (int c = 0; c < kTurnLd; ++c) {
      const int want = c < 32 ? 1 : 0;                 // the 4 pad columns are never touched
      CHECK(written[row * kTurnLd + c] == want && read[row * kTurnLd + c] == want);
    }
  CHECK(turn_bytes(8) == 8 * 32 * kTurnLd * 4 && kTurnLd % 4 == 0 && kTurnLd % 32 != 0);
}

static void check_mfma32_row() {
  std::set<int> rows;
  for (int kl = 0; kl < 2; ++kl) {
    int prev = -1;
    for (int r = 0; r < 16; ++r) {
      const int row = mfma32_row(r, kl);
      CHECK(row >= 0 && row < 32 && row > prev);      // ascending in r
      prev = row;
      rows.insert(row);
    }
  }
  CHECK(rows.size() == 32);
}

int main() {
  for (int rows : {64, 128, 192, 256, 320, 384}) check_chunk_image(32, rows);      // tiles of the general and persistent kernels (A + B rows)
  for (int rows : {64, 128, 256}) check_chunk_image(16, rows);
  check_stream_image(128);
  check_stream_image(256);
  check_turn_round();
  check_mfma32_row();
  std::printf(failures ? "%d checks failed\n" : "f16x3 layout: all checks passed\n", failures);
  return failures ? 1 : 0;
}
