// Stand-alone CPU check of the host index arithmetic of csrc/units_fit.hip (units_fit_layout.h): build it with a host compiler and
// -fsanitize=address,undefined and run it; it needs no GPU and no HIP.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I unitspeech_amd/csrc tools/units_fit_layout_check.cpp -o /tmp/layout_check && /tmp/layout_check
//
// For a grid of (rows, K, D) it checks that the sections of the state and of the workspace are 16-byte aligned, in order and inside the
// total, writes the first and last byte of every section of a real allocation of that size, replays the inverted index on the host
// (histogram [k][chunk], exclusive scan, stable scatter, item table) for several labellings and checks every index the kernels form:
// list positions inside [0, rows), ascending rows per centre, work items inside max_items.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "units_fit_layout.h"

using namespace us::fit;

static int failures = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAILED %s (line %d)\n", #c, __LINE__);               \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static void touch(std::vector<unsigned char>& buf, size_t begin, size_t end) {
  CHECK(begin % 16 == 0 && begin <= end && end <= buf.size());
  if (begin < end) {
    buf[begin] = 1;
    buf[end - 1] = 1;
  }
}

static void check_layouts(int64_t rows, int K, int D, bool allocate) {
  const StateLayout s = state_layout(K, D);
  CHECK(s.sums == 0 && s.sums < s.counts && s.counts < s.shift && s.shift < s.scalars && s.scalars + 32 == s.total);
  CHECK(s.counts - s.sums >= (size_t)K * D * 8 && s.shift - s.counts >= (size_t)K * 8 && s.scalars - s.shift >= (size_t)K * 8);
  const WorkLayout w = work_layout(rows, K, D);
  const IndexDims d = index_dims(rows, K);
  CHECK(d.nchunks >= 1 && (int64_t)d.nchunks * kRowChunk >= rows && (int64_t)(d.nchunks - 1) * kRowChunk < rows);
  CHECK((int64_t)d.nscan * kScanItems >= d.m && d.m == (int64_t)K * d.nchunks);
  CHECK(d.m + 1 <= INT32_MAX && d.max_items <= INT32_MAX && rows <= INT32_MAX);
  const size_t order[] = {w.offs, w.bsum, w.skip, w.index, w.cstart, w.part, w.pin, w.seed_sum, w.seed_cnt, w.seed_sel, w.total};
  const size_t need[] = {(size_t)(d.m + 1) * 4, (size_t)d.nscan * 4, (size_t)d.nchunks * 4, (size_t)rows * 4, (size_t)(K + 1) * 4,
                         (size_t)d.max_items * D * 8, (size_t)d.max_items * 8, (size_t)ceil_div(rows, kSeedBlock) * 8,
                         (size_t)ceil_div(rows, kSeedBlock) * 4, 48};
  for (int i = 0; i < 10; ++i) CHECK(order[i] % 16 == 0 && order[i] + need[i] <= order[i + 1]);
  if (allocate) {
    std::vector<unsigned char> ws(w.total), st(s.total);
    for (int i = 0; i < 10; ++i) touch(ws, order[i], order[i] + need[i]);
    touch(st, s.sums, s.sums + (size_t)K * D * 8);
    touch(st, s.counts, s.counts + (size_t)K * 8);
    touch(st, s.shift, s.shift + (size_t)K * 8);
    touch(st, s.scalars, s.scalars + 32);
  }
}

// the inverted index as the kernels build it, on the host
static void replay(int64_t rows, int K, const std::vector<long long>& labels) {
  const IndexDims d = index_dims(rows, K);
  std::vector<int> offs(d.m + 1, 0), index(rows, -1), cstart(K + 1, 0);
  for (int64_t r = 0; r < rows; ++r) {
    const long long l = labels[r];
    if (l >= 0 && l < K) ++offs[(size_t)l * d.nchunks + r / kRowChunk];
  }
  int run = 0;
  for (int64_t i = 0; i < d.m; ++i) {
    const int v = offs[i];
    offs[i] = run;
    run += v;
  }
  offs[d.m] = run;
  CHECK(run <= rows);
  for (int c = 0; c < d.nchunks; ++c) {
    for (int k = 0; k < K; ++k) {
      int pos = offs[(size_t)k * d.nchunks + c];
      const int end = offs[(size_t)k * d.nchunks + c + 1];
      for (int i = 0; i < kRowChunk; ++i) {
        const int64_t r = (int64_t)c * kRowChunk + i;
        if (r < rows && labels[r] == k && pos < end) {
          CHECK(pos >= 0 && pos < rows);
          index[pos++] = (int)r;
        }
      }
      CHECK(pos == end);
    }
  }
  int items = 0;
  for (int k = 0; k < K; ++k) {
    cstart[k] = items;
    const int beg = offs[(size_t)k * d.nchunks], end = offs[(size_t)(k + 1) * d.nchunks];
    items += (end - beg + kListChunk - 1) / kListChunk;
    for (int p = beg; p < end; ++p) {
      CHECK(index[p] >= 0 && index[p] < rows && labels[index[p]] == k);
      if (p > beg) CHECK(index[p] > index[p - 1]);
    }
  }
  cstart[K] = items;
  CHECK(items <= d.max_items);
  for (int w = 0; w < items; ++w) {                       // the work item -> (centre, piece) search of the gather kernel
    int lo = 0, hi = K;
    for (int it = 0; it < 12 && hi - lo > 1; ++it) {
      const int mid = (lo + hi) >> 1;
      if (cstart[mid] <= w) lo = mid; else hi = mid;
    }
    const int k = lo, j = w - cstart[k];
    const int beg = offs[(size_t)k * d.nchunks] + j * kListChunk, end = offs[(size_t)(k + 1) * d.nchunks];
    CHECK(cstart[k] <= w && w < cstart[k + 1] && beg < end && beg >= 0 && end <= rows);
  }
}

int main() {
  const int64_t row_sizes[] = {1, 70, 511, 512, 513, 1023, 1024, 1025, 3000, 4096, 20000, 65537, 200000, kMaxRows};
  const int ks[] = {1, 2, 37, 255, 256, 257, 1000, 2048};
  const int ds[] = {4, 36, 256, 260, 768, 1024};
  for (int64_t rows : row_sizes)
    for (int K : ks)
      for (int D : ds) check_layouts(rows, K, D, rows <= 20000 && (int64_t)K * D <= 64 * 1024);
  CHECK(!shape_ok(0, 4) && !shape_ok(2049, 4) && !shape_ok(8, 0) && !shape_ok(8, 770) && !shape_ok(8, 1028) && shape_ok(2048, 1024));
  CHECK(!rows_ok(0) && !rows_ok(kMaxRows + 1) && rows_ok(kMaxRows));
  std::mt19937 g(1);
  for (int64_t rows : {1, 70, 513, 1025, 3000, 20000}) {
    for (int K : {1, 8, 37, 257, 2048}) {
      std::vector<long long> even(rows), skew(rows), odd(rows);
      for (int64_t r = 0; r < rows; ++r) {
        even[r] = (long long)(g() % K);
        skew[r] = g() % 10 ? 0 : (long long)(g() % K);
        odd[r] = (long long)(g() % (K + 3)) - 2;          // -2, -1 and K are skipped rows
      }
      replay(rows, K, even);
      replay(rows, K, skew);
      replay(rows, K, odd);
      replay(rows, K, std::vector<long long>(rows, -1));
      replay(rows, K, std::vector<long long>(rows, K - 1));
    }
  }
  std::printf(failures ? "%d checks failed\n" : "units_fit layout: all checks passed\n", failures);
  return failures ? 1 : 0;
}
