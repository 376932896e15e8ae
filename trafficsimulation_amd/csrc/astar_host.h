// astar_host.h - the wave searcher's algorithm (astar.h: astar_wave / astar_loop<*, true, false>) as a sequential host function, and
// the persistent thread pool that runs a batch of such searches.  Plain C++17 without HIP, so that a stand-alone program can
// compile it (tests/native/astar_host_check.cpp); the engine includes it from engine.hip and finishes the last long searches of a
// replanning pass with it (replan_host.h).
//
// A search reads a host copy of the A* snapshot (Dev::amap, k_amap_build's words in 8 x 8-tiled order) and keeps k_replan's table
// record: both layouts, and the costs in half units, are astar_words.h.  It covers searches in half units
// without a field-of-view mask - what astar_half_units(P) && !respect_awareness selects on the device - and restates them quirk for
// quirk (astar_numba.py:87-239 as astar.h lists it): an f-only binary heap with strict '<' in both sifts, dir_arr in heap-slot order and
// not moved by the sifts, relaxations in the order N, E, S, W, `ng` truncated when stored.  n_exp / n_relax count what the device
// counts: fresh pops and committed relaxations.
#pragma once
#ifdef __linux__
#include <sched.h>
#endif
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>
#include "astar_words.h"

namespace ahost {

constexpr uint32_t STAMP_MAX = (1u << (32 - W_STAMP_SHIFT)) - 1u;   // a searcher's own epochs: every stamp the meta word holds

struct Costs { HalfCosts hc; bool turn_on, rt_on; };     // TsParams' penalties in half units, and the two switches
inline Costs costs_of(const TsParams& P) { return Costs{half_costs(P), P.turn_penalty_enabled != 0, P.road_type_penalties_enabled != 0}; }
struct Map {
  const uint64_t* amap;
  int W, H, W8, N;
  uint32_t n_nodes;
  int heap_cap;      // a heap that would outgrow it ends the search with -1, as on the device (ASlots::heap_cap)
};
struct Query { int start, goal; bool soft, ignore_flow; int maximum_steps; };
struct Result { int len; int n_exp, n_relax; };     // len: cells written (start excluded, goal included), 0 = no path, -1 = heap / path buffer exceeded

class Searcher {
 public:
  // One search; the path goes to out[0..len).  The table (one record per node, stamped with an epoch: no clear per call) and
  // the heap are kept between calls.
  Result run(const Map& m, const Costs& c, const Query& q, int32_t* out, int out_cap) {
    if (tab_.size() != (size_t)m.n_nodes + 1) { tab_.assign((size_t)m.n_nodes + 1, 0ull); epoch_ = 0; }
    if (++epoch_ > STAMP_MAX) { std::fill(tab_.begin(), tab_.end(), 0ull); epoch_ = 1; }
    const uint32_t epoch = epoch_;
    const uint64_t* amap = m.amap;
    uint64_t* tab = tab_.data();
    const int W = m.W, H = m.H, W8 = m.W8;
    // (tables for the loops below, filled from the header's definitions: compares per neighbour cost tests/native/astar_host_check 3 %)
    const int rt2[4] = {0, c.hc.rt2_1, c.hc.rt2_2, c.hc.rt2_3};
    const int DX[4] = {dir_dx(0), dir_dx(1), dir_dx(2), dir_dx(3)}, DY[4] = {dir_dy(0), dir_dy(1), dir_dy(2), dir_dy(3)};
    const int sx = q.start % W, sy = q.start / W, gx = q.goal % W, gy = q.goal / W;
    const int goal_xy = (gy << 16) | gx;
    const bool limited = q.maximum_steps < m.N;
    Result r{0, 0, 0};
    {
      const uint32_t sr = am_node(amap[tix(W8, sx, sy)]);
      if (sr != AM_NO_NODE) tab[sr] = tent_word(0, epoch, 0u, 0u);      // dist 0, steps 0
    }
    hq_.clear(); hd_.clear();
    hq_.push_back(HQ{std::abs(sx - gx) + std::abs(sy - gy), (sy << 16) | sx});
    hd_.push_back(-1);
    while (!hq_.empty()) {
      const HQ top = hq_[0];
      const int prev_dir = hd_[0];
      {  // heap_pop: the last entry takes the root's place (its dir byte with it) and sinks; ties go to it, then to the left child
        const HQ x = hq_.back();
        const int8_t xd = hd_.back();
        hq_.pop_back(); hd_.pop_back();
        const int n = (int)hq_.size();
        if (n > 0) {
          hd_[0] = xd;
          HQ* h = hq_.data();
          int idx = 0;
          for (;;) {
            const int l = 2 * idx + 1;
            if (l >= n) break;
            int ch = l, cf = h[l].f;
            if (l + 1 < n && h[l + 1].f < cf) { ch = l + 1; cf = h[l + 1].f; }
            if (!(cf < x.f)) break;
            h[idx] = h[ch];
            idx = ch;
          }
          h[idx] = x;
        }
      }
      const int cur = top.i, cx = cur & 0xFFFF, cy = (int)((uint32_t)cur >> 16);
      const uint64_t am_c = amap[tix(W8, cx, cy)];
      if (cur == goal_xy) {
        // walk came_from back to the start, filling the output from its far end, then slide it to the front
        int len = 0, px = cx, py = cy;
        for (int cc = cy * W + cx; cc != q.start;) {
          if (len >= out_cap) { r.len = -1; return r; }
          out[out_cap - 1 - len] = cc;
          len++;
          const int dd = tent_dir(tab[am_node(amap[tix(W8, px, py)])]);
          px -= DX[dd]; py -= DY[dd];
          cc = py * W + px;
        }
        const int shift = out_cap - len;
        if (shift > 0) for (int k = 0; k < len; k++) out[k] = out[shift + k];
        r.len = len;
        return r;
      }
      const int g = top.f - (std::abs(cx - gx) + std::abs(cy - gy));
      const uint32_t r_c = am_node(am_c);
      int dist_c = 0, steps = 0;
      if (r_c != AM_NO_NODE) {       // (only a start cell can be off the node set: dist 0, no steps)
        const uint64_t e_c = tab[r_c];
        dist_c = tent_dist(e_c, epoch);
        steps = limited ? tent_steps(e_c) : 0;
      }
      if (!(g <= dist_c)) continue;      // a stale pop relaxes nothing
      r.n_exp++;
      if (steps + 1 > q.maximum_steps) continue;
      const uint32_t bits = am_dirs((uint32_t)am_c);
      for (int dd = 0; dd < 4; dd++) {
        const int nx = cx + DX[dd], ny = cy + DY[dd];
        if ((unsigned)nx >= (unsigned)W || (unsigned)ny >= (unsigned)H) continue;
        const uint64_t am = amap[tix(W8, nx, ny)];
        const uint32_t a = (uint32_t)am, rn = am_node(am);
        if (rn == AM_NO_NODE) continue;
        const bool n_occ = am_occ(a), n_stop = am_red(a), n_road = am_road(a);
        const bool flow = ((bits >> dd) & 1u) != 0u;
        if (!(flow | (q.ignore_flow & n_road))) continue;
        if (!(q.soft | !(n_occ | n_stop))) continue;
        int n2 = 2 * (g + 1);
        n2 += (c.turn_on & (prev_dir != -1) & (dd != prev_dir)) ? c.hc.turn2 : 0;
        n2 += flow ? 0 : c.hc.contra2;
        n2 += n_occ ? am_pen2(a) : 0;
        n2 += n_stop ? c.hc.stop2 : 0;
        n2 += (c.rt_on & n_road) ? rt2[am_road_type(a)] : 0;
        const int dist_n = tent_dist(tab[rn], epoch);
        if (!(n2 < 2 * dist_n)) continue;
        // (the four neighbours are distinct cells: committing one changes no other one's test)
        if ((int)hq_.size() + 1 > m.heap_cap) { r.len = -1; return r; }
        r.n_relax++;
        const int ngi = n2 >> 1;
        tab[rn] = tent_word(ngi, epoch, limited ? (uint32_t)(steps + 1) : 0u, (uint32_t)dd);
        const HQ ne{ngi + std::abs(nx - gx) + std::abs(ny - gy), (ny << 16) | nx};
        // heap_push: the dir byte stays in the slot the entry was appended to, the entry rises past every ancestor with a larger key
        int i = (int)hq_.size();
        hq_.push_back(ne);
        hd_.push_back((int8_t)dd);
        HQ* h = hq_.data();
        while (i > 0) {
          const int p = (i - 1) >> 1;
          if (!(ne.f < h[p].f)) break;
          h[i] = h[p];
          i = p;
        }
        h[i] = ne;
      }
    }
    return r;
  }

 private:
  struct HQ { int32_t f, i; };      // heap entry: key, cell as y << 16 | x
  std::vector<uint64_t> tab_;       // per node: k_replan's table record (tent_word)
  uint32_t epoch_ = 0;
  std::vector<HQ> hq_;
  std::vector<int8_t> hd_;
};

// threads a pool may use: the cores this process may run on, sixteen at the most (never the machine's core count)
inline int pool_default_threads() {
  int n = 1;
#ifdef __linux__
  cpu_set_t set;
  CPU_ZERO(&set);
  if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
#endif
  return n < 1 ? 1 : n > 16 ? 16 : n;
}

// Persistent workers, each with a Searcher of its own; run() hands out the items of a batch one by one and returns when all are done.
class Pool {
 public:
  explicit Pool(int threads) : searchers_((size_t)(threads < 1 ? 1 : threads)) {
    for (size_t t = 0; t < searchers_.size(); t++) workers_.emplace_back([this, t]() { work((int)t); });
  }
  ~Pool() {
    { std::lock_guard<std::mutex> lk(mu_); quit_ = true; }
    cv_.notify_all();
    for (auto& w : workers_) w.join();
  }
  Pool(const Pool&) = delete;
  Pool& operator=(const Pool&) = delete;
  int threads() const { return (int)searchers_.size(); }
  // fn(searcher, item) for item = 0 .. n - 1, on at most `use` threads (0: all)
  void run(int n, const std::function<void(Searcher&, int)>& fn, int use = 0) {
    if (n <= 0) return;
    std::unique_lock<std::mutex> lk(mu_);
    fn_ = &fn; n_ = n; next_.store(0, std::memory_order_relaxed);
    use_ = use <= 0 || use > threads() ? threads() : use;
    left_ = use_;
    gen_++;
    cv_.notify_all();
    done_cv_.wait(lk, [this]() { return left_ == 0; });
    fn_ = nullptr;
  }

 private:
  void work(int t) {
    std::unique_lock<std::mutex> lk(mu_);
    unsigned seen = 0;
    for (;;) {
      cv_.wait(lk, [&]() { return gen_ != seen || quit_; });
      if (quit_) return;
      seen = gen_;
      if (t >= use_) continue;
      const std::function<void(Searcher&, int)>* fn = fn_;
      const int n = n_;
      lk.unlock();
      for (int k; (k = next_.fetch_add(1, std::memory_order_relaxed)) < n;) (*fn)(searchers_[(size_t)t], k);
      lk.lock();
      if (--left_ == 0) done_cv_.notify_all();
    }
  }
  std::vector<Searcher> searchers_;
  std::vector<std::thread> workers_;
  std::mutex mu_;
  std::condition_variable cv_, done_cv_;
  const std::function<void(Searcher&, int)>* fn_ = nullptr;
  std::atomic<int> next_{0};
  int n_ = 0, use_ = 0, left_ = 0;
  unsigned gen_ = 0;
  bool quit_ = false;
};

}  // namespace ahost
