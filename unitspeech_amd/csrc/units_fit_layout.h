// Host-side index arithmetic of csrc/units_fit.hip: the limits, the state and workspace layouts and the sizes of the inverted index's
// tables.  Plain C++ with no device code, so that a stand-alone CPU program can walk it (tools/units_fit_layout_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace us {
namespace fit {

constexpr int kMaxK = 2048, kMaxD = 1024;
constexpr int64_t kMaxRows = 1LL << 24;   // per call
constexpr int kRowChunk = 1024;           // rows per histogram chunk (one workgroup stages its labels in LDS)
constexpr int kListChunk = 512;           // rows of one centre's list that one wave sums
constexpr int kScanItems = 4096;          // entries per workgroup of the blocked scan (256 threads x 16)
constexpr int kSeedBlock = 1024;          // rows per block of the seeding's blocked scan (256 threads x 4)

inline bool shape_ok(int K, int D) { return K >= 1 && K <= kMaxK && D >= 4 && D <= kMaxD && D % 4 == 0; }
inline bool rows_ok(int64_t rows) { return rows >= 1 && rows <= kMaxRows; }
inline size_t align16(size_t v) { return (v + 15) / 16 * 16; }
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The state several accumulate calls add into: fp64 sums [K][D] | int64 counts [K] | fp64 shift partials [K] |
// scalars {fp64 inertia, int64 rows used, int64 rows skipped, int64 spare}.
struct StateLayout {
  size_t sums, counts, shift, scalars, total;
};
inline StateLayout state_layout(int K, int D) {
  StateLayout l;
  size_t o = 0;
  l.sums = o;
  o += align16((size_t)K * D * sizeof(double));
  l.counts = o;
  o += align16((size_t)K * sizeof(int64_t));
  l.shift = o;
  o += align16((size_t)K * sizeof(double));
  l.scalars = o;
  o += 4 * sizeof(int64_t);
  l.total = o;
  return l;
}

// Sizes of the inverted index of one accumulate call.
struct IndexDims {
  int nchunks;        // row chunks
  int64_t m;          // histogram entries: K x nchunks, laid out [k][chunk] so that one exclusive scan places every (centre, chunk)
  int nscan;          // workgroups of the blocked scan over m entries
  int64_t max_items;  // upper bound on (centre, list chunk) work items: sum_k ceil(count_k / kListChunk) <= K + rows / kListChunk
};
inline IndexDims index_dims(int64_t rows, int K) {
  IndexDims d;
  d.nchunks = (int)ceil_div(rows, kRowChunk);
  d.m = (int64_t)K * d.nchunks;
  d.nscan = (int)ceil_div(d.m, kScanItems);
  d.max_items = (int64_t)K + rows / kListChunk;
  return d;
}

// Workspace: [accumulate: offs (m + 1) | scan block sums | skipped per chunk | row index | item table (K + 1) | partial sums | partial
// inertia] [seeding: block sums fp64 | block counts | selection record].
struct WorkLayout {
  size_t offs, bsum, skip, index, cstart, part, pin, seed_sum, seed_cnt, seed_sel, total;
};
inline WorkLayout work_layout(int64_t rows, int K, int D) {
  const IndexDims d = index_dims(rows, K);
  const int64_t nseed = ceil_div(rows, kSeedBlock);
  WorkLayout l;
  size_t o = 0;
  l.offs = o;
  o += align16((size_t)(d.m + 1) * sizeof(int32_t));
  l.bsum = o;
  o += align16((size_t)d.nscan * sizeof(int32_t));
  l.skip = o;
  o += align16((size_t)d.nchunks * sizeof(int32_t));
  l.index = o;
  o += align16((size_t)rows * sizeof(int32_t));
  l.cstart = o;
  o += align16((size_t)(K + 1) * sizeof(int32_t));
  l.part = o;
  o += align16((size_t)d.max_items * D * sizeof(double));
  l.pin = o;
  o += align16((size_t)d.max_items * sizeof(double));
  l.seed_sum = o;
  o += align16((size_t)nseed * sizeof(double));
  l.seed_cnt = o;
  o += align16((size_t)nseed * sizeof(int32_t));
  l.seed_sel = o;
  o += 64;
  l.total = o;
  return l;
}

}  // namespace fit
}  // namespace us
