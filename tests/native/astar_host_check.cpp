// The host searcher (csrc/astar_host.h) against recorded answers, as a plain executable: tests/test_host_astar_native.py writes one
// case file per world (the A* snapshot words, the cost constants, the queries and the reference's paths) and runs this program on
// them - plain, under AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer.  Every query runs once on a single
// Searcher and eight times on a pool of four threads; every path must equal the recorded one cell for cell.
//
// Case file, int32 words: 'ASTH', W, H, n_nodes, heap_cap, turn_on, rt_on, turn2, contra2, stop2, rt2_1, rt2_2, rt2_3, n_queries,
// n_path_cells; then W8 * H8 * 64 uint64 snapshot words; n_queries x 7 (sx, sy, gx, gy, soft, ignore_flow, maximum_steps);
// n_queries + 1 path offsets; n_path_cells x 2 (x, y).
#include <cstdio>
#include <cstring>
#include <string>

#include "astar_host.h"

namespace {

struct Case {
  int W = 0, H = 0;
  ahost::Map map{};
  ahost::Costs costs{};
  std::vector<uint64_t> amap;
  std::vector<int32_t> queries, off, xy;
  int nq = 0;
};

bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

bool load(const char* path, Case& c) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  int32_t h[15];
  bool ok = read_all(f, h, sizeof(h)) && h[0] == 0x48545341 && h[1] > 0 && h[2] > 0 && h[3] >= 0 && h[13] >= 0 && h[14] >= 0;
  if (ok) {
    c.W = h[1]; c.H = h[2];
    const int W8 = (c.W + 7) / 8, H8 = (c.H + 7) / 8;
    c.amap.resize((size_t)W8 * H8 * 64);
    c.nq = h[13];
    c.queries.resize((size_t)c.nq * 7); c.off.resize((size_t)c.nq + 1); c.xy.resize((size_t)h[14] * 2);
    ok = read_all(f, c.amap.data(), c.amap.size() * 8) && read_all(f, c.queries.data(), c.queries.size() * 4) &&
         read_all(f, c.off.data(), c.off.size() * 4) && read_all(f, c.xy.data(), c.xy.size() * 4);
    c.map = ahost::Map{c.amap.data(), c.W, c.H, W8, c.W * c.H, (uint32_t)h[3], h[4]};
    c.costs = ahost::Costs{HalfCosts{h[7], h[8], 0, h[9], h[10], h[11], h[12]}, h[5] != 0, h[6] != 0};   // (veh2: in the snapshot words)
    ok = ok && c.off[0] == 0 && c.off[c.nq] == h[14];
  }
  fclose(f);
  return ok;
}

// query k of the case on searcher s: empty string when the path is the recorded one
std::string check_query(const Case& c, ahost::Searcher& s, int k, std::vector<int32_t>& buf) {
  const int32_t* q = &c.queries[(size_t)k * 7];
  buf.resize((size_t)c.W * c.H);
  const ahost::Query qu{q[1] * c.W + q[0], q[3] * c.W + q[2], q[4] != 0, q[5] != 0, q[6]};
  const ahost::Result r = s.run(c.map, c.costs, qu, buf.data(), (int)buf.size());
  const int want = c.off[k + 1] - c.off[k];
  if (r.len != want) return "query " + std::to_string(k) + ": length " + std::to_string(r.len) + ", recorded " + std::to_string(want);
  for (int j = 0; j < want; j++) {
    const int x = c.xy[2 * ((size_t)c.off[k] + j)], y = c.xy[2 * ((size_t)c.off[k] + j) + 1];
    if (buf[j] != y * c.W + x) return "query " + std::to_string(k) + ": cell " + std::to_string(j) + " differs";
  }
  if (r.n_exp < 0 || r.n_relax < r.n_exp - 1) return "query " + std::to_string(k) + ": counters " + std::to_string(r.n_exp) + " / " + std::to_string(r.n_relax);
  return "";
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: astar_host_check CASE...\n"); return 2; }
  int total = 0;
  ahost::Searcher single;          // one searcher over every world: its table is rebuilt when the node count changes
  ahost::Pool pool(4);
  for (int a = 1; a < argc; a++) {
    Case c;
    if (!load(argv[a], c)) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
    std::vector<int32_t> buf;
    for (int k = 0; k < c.nq; k++) {
      const std::string err = check_query(c, single, k, buf);
      if (!err.empty()) { printf("%s single-threaded, %s\n", argv[a], err.c_str()); return 1; }
    }
    // every query eight times, on four threads: item j is query j % nq
    std::mutex mu;
    std::string first_err;
    pool.run(c.nq * 8, [&](ahost::Searcher& s, int j) {
      thread_local std::vector<int32_t> tbuf;
      const std::string err = check_query(c, s, j % c.nq, tbuf);
      if (!err.empty()) { std::lock_guard<std::mutex> lk(mu); if (first_err.empty()) first_err = err; }
    });
    if (!first_err.empty()) { printf("%s on the pool, %s\n", argv[a], first_err.c_str()); return 1; }
    total += c.nq;
  }
  printf("astar host ok: %d queries, each once single-threaded and eight times on %d threads\n", total, pool.threads());
  return 0;
}
