// The walk, pool and ranking logic of Whisper's beam search (openai-whisper's BeamSearchDecoder.update / finalize and
// MaximumLikelihoodRanker with length_penalty=None, as tools/whisper_beam_numpy.py states them), for host and device: whisper.hip's
// wh_beam_book_kernel and wh_beam_final_kernel call these from one thread of an item's workgroup, and tools/whisper_beam_check.cpp walks
// them on the CPU under the sanitizers.  Plain functions over caller-owned arrays; nothing is allocated and every loop is bounded by its
// arguments.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WB_HD __host__ __device__
#else
#define WB_HD
#endif

namespace us {

constexpr int kWbMaxBeam = 16;                                  // rows of an item
constexpr int kWbMaxCands = kWbMaxBeam * (kWbMaxBeam + 1);      // every row offers at most beam + 1 candidates
constexpr int kWbMaxPool = 64;                                  // max_candidates; the pool's capacity is max(C, n) <= 64

struct WbRow {                  // a new row: the row it continues, its token, its score
  int parent, token;
  double score;
};
struct WbFin {                  // a newly finished entry, in walk order: the row whose sequence it is (stored without the eos), its score
  int parent;
  double score;
};
struct WbWalk {
  int rows, finished, added, walked;    // new rows, newly finished, how many of those the pool takes, candidates looked at
  int ended;                            // the pool holds C entries, or no row is live
};

// the place of candidate c in the list sorted descending by total, equal totals in index order (a stable sort, by counting)
WB_HD inline int wb_rank(const double* total, int count, int c) {
  int r = 0;
  for (int o = 0; o < count; ++o) r += total[o] > total[c] || (total[o] == total[c] && o < c) ? 1 : 0;
  return r;
}

// order[r]: the candidate at place r.  Candidate c is (parent[c], token[c], total[c]), listed in (row, rank) order.  The walk stops as soon
// as n new rows exist; everything behind the stop is ignored.  rows: [n], fin: [count].
WB_HD inline WbWalk wb_walk(const int* order, const int* parent, const int* token, const double* total, int count, int n, int C, int eos,
                            int pool, WbRow* rows, WbFin* fin) {
  WbWalk w{0, 0, 0, 0, 0};
  for (int r = 0; r < count && w.rows < n; ++r) {
    const int c = order[r];
    ++w.walked;
    if (token[c] == eos) fin[w.finished++] = WbFin{parent[c], total[c]};
    else rows[w.rows++] = WbRow{parent[c], token[c], total[c]};
  }
  const int room = C - pool;
  w.added = room <= 0 ? 0 : (w.finished < room ? w.finished : room);
  w.ended = pool + w.added >= C || w.rows == 0 ? 1 : 0;
  return w;
}

// finalise: the live rows a pool of `pool` < n entries takes, in descending score, the lower row first on a tie -> out[], their count
WB_HD inline int wb_top_up(const int* live, const double* score, int n, int pool, int* out) {
  int k = 0;
  for (; pool + k < n; ++k) {
    int best = -1;
    for (int j = 0; j < n; ++j) {
      if (!live[j]) continue;
      bool used = false;
      for (int u = 0; u < k; ++u) used = used || out[u] == j;
      if (!used && (best < 0 || score[j] > score[best])) best = j;
    }
    if (best < 0) break;
    out[k] = best;
  }
  return k;
}

// the ranker: the entry with the largest score / length (length 0: -infinity), the earlier one on a tie; count >= 1
WB_HD inline int wb_winner(const double* score, const int* length, int count) {
  int best = 0;
  bool has = length[0] > 0;
  double bv = has ? score[0] / (double)length[0] : 0.0;
  for (int i = 1; i < count; ++i) {
    if (length[i] <= 0) continue;
    const double v = score[i] / (double)length[i];
    if (!has || v > bv) {
      best = i;
      bv = v;
      has = true;
    }
  }
  return best;
}

}  // namespace us
