// The beam-search bookkeeping of csrc/whisper_beam.h on the CPU: the functions wh_beam_book_kernel and wh_beam_final_kernel call, over cases
// read as text from a file (argv[1]) or stdin, results printed one line per case.  tests/test_whisper_beam.py builds this with
// -fsanitize=address,undefined and compares the lines with tools/whisper_beam_numpy.py.
//
//   S n C eos pool          one step: then n rows `live score count` each followed by count pairs `token logprob`, the row's candidates
//                           in rank order
//     -> S rows K {parent token score} fin M {parent score} added A walked W ended E
//   F n pool                finalise and rank: then pool entries `score length`, then n rows `live score length`
//     -> F top K {row} winner I       (I indexes the pool followed by the topped-up rows)
//
//   c++ -std=c++17 -fsanitize=address,undefined -I unitspeech_amd/csrc tools/whisper_beam_check.cpp -o whisper_beam_check
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "whisper_beam.h"

using namespace us;

static int fail(const char* what) {
  std::fprintf(stderr, "whisper_beam_check: %s\n", what);
  return 2;
}

int main(int argc, char** argv) {
  std::ifstream file;
  if (argc > 1) {
    file.open(argv[1]);
    if (!file) return fail("cannot open the case file");
  }
  std::istream& in = argc > 1 ? static_cast<std::istream&>(file) : std::cin;
  std::string kind;
  int cases = 0;
  while (in >> kind) {
    if (kind == "S") {
      int n, C, eos, pool;
      if (!(in >> n >> C >> eos >> pool) || n < 1 || n > kWbMaxBeam || C < 1 || C > kWbMaxPool || pool < 0) return fail("bad step header");
      std::vector<int> parent, token;
      std::vector<double> total;
      for (int j = 0; j < n; ++j) {
        int live, count;
        double score;
        if (!(in >> live >> score >> count) || count < 0 || count > n + 1) return fail("bad row");
        for (int k = 0; k < count; ++k) {
          int tok;
          double lp;
          if (!(in >> tok >> lp)) return fail("bad candidate");
          if (!live) continue;
          parent.push_back(j);
          token.push_back(tok);
          total.push_back(score + lp);
        }
      }
      const int count = (int)total.size();
      std::vector<int> order(count);
      for (int c = 0; c < count; ++c) order[wb_rank(total.data(), count, c)] = c;
      std::vector<WbRow> rows(n);
      std::vector<WbFin> fin(count + 1);
      const WbWalk w = wb_walk(order.data(), parent.data(), token.data(), total.data(), count, n, C, eos, pool, rows.data(), fin.data());
      std::printf("S rows %d", w.rows);
      for (int k = 0; k < w.rows; ++k) std::printf(" %d %d %.17g", rows[k].parent, rows[k].token, rows[k].score);
      std::printf(" fin %d", w.finished);
      for (int k = 0; k < w.finished; ++k) std::printf(" %d %.17g", fin[k].parent, fin[k].score);
      std::printf(" added %d walked %d ended %d\n", w.added, w.walked, w.ended);
    } else if (kind == "F") {
      int n, pool;
      if (!(in >> n >> pool) || n < 1 || n > kWbMaxBeam || pool < 0 || pool > kWbMaxPool) return fail("bad finalise header");
      std::vector<double> score(pool), rscore(n);
      std::vector<int> length(pool), live(n), rlen(n), top(n);
      for (int i = 0; i < pool; ++i)
        if (!(in >> score[i] >> length[i])) return fail("bad pool entry");
      for (int j = 0; j < n; ++j)
        if (!(in >> live[j] >> rscore[j] >> rlen[j])) return fail("bad row");
      const int k = wb_top_up(live.data(), rscore.data(), n, pool, top.data());
      for (int u = 0; u < k; ++u) {
        score.push_back(rscore[top[u]]);
        length.push_back(rlen[top[u]]);
      }
      std::printf("F top %d", k);
      for (int u = 0; u < k; ++u) std::printf(" %d", top[u]);
      if (score.empty()) return fail("an empty pool and no live row");
      std::printf(" winner %d\n", wb_winner(score.data(), length.data(), (int)score.size()));
    } else {
      return fail("a case starts with S or F");
    }
    ++cases;
  }
  std::fprintf(stderr, "whisper_beam_check: %d cases\n", cases);
  return 0;
}
