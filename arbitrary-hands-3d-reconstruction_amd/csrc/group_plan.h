// Which ops of a program share a launch: the rule of the executor's grouped launches (acrmi_program.hip build_schedule; the
// launch itself: conv_frame.h ConvGroup).  Plain C++17, host only, no HIP header: tools/group_plan_check.cpp runs it on a
// lowered program without a device.
//
// A group is a run of ops that
//   (a) the routing sends to ONE kernel instantiation with a group form (`same`, asked of the launchers),
//   (b) have no dependency edge between them (the edges are the RAW / WAR / WAW hazards on buffer ids, so two ops whose
//       buffers alias through lifetime reuse have one),
//   (c) sit on one lane - by construction: a follower takes its leader's lane (build_schedule),
//   (d) are adjacent in the enqueue order, or can be made adjacent without crossing an edge: an op further down the order
//       may move up to its leader when it depends on nothing in between.
// HRNet is why (d) matters: the lowering emits a module branch by branch, so branch 1's and branch 2's convolutions of one
// depth - independent, on the same kernel - lie eight ops apart, each depending only on its own branch.
#pragma once
#include <algorithm>
#include <vector>

namespace acrmi {

// How far down the order a partner is looked for (two branches of four basic blocks are 8 ops apart; the margin is for the
// ops a lowering may put between them).
constexpr int GROUP_LOOKAHEAD = 16;

// deps[j] = the earlier ops j must wait for, from the buffers each op reads / writes, in `order` (a topological order).
// n_ops / n_bufs size the tables; ops outside `order` get no edges.
inline std::vector<std::vector<int>> hazard_deps(const std::vector<int>& order, const std::vector<std::vector<int>>& reads,
                                                 const std::vector<std::vector<int>>& writes, int n_ops, int n_bufs) {
  std::vector<std::vector<int>> deps(n_ops);
  std::vector<int> last_writer(n_bufs, -1);
  std::vector<std::vector<int>> readers(n_bufs);
  for (int j : order) {
    std::vector<int>& d = deps[j];
    auto dep = [&](int i) { if (i >= 0 && i != j && std::find(d.begin(), d.end(), i) == d.end()) d.push_back(i); };
    for (int b : reads[j]) dep(last_writer[b]);
    for (int b : writes[j]) { dep(last_writer[b]); for (int i : readers[b]) dep(i); }
    for (int b : reads[j]) readers[b].push_back(j);
    for (int b : writes[j]) { last_writer[b] = j; readers[b].clear(); }
  }
  return deps;
}

// Forms the groups and moves every follower behind its leader in `order` (still a topological order of `deps`).
// leader[j] = j for an op that launches (alone or as the first of its group), else the op whose launch runs j.
// same(x, y): x and y go to one instantiation with a group form; gmax: ops per group.
template <class Same>
inline std::vector<int> plan_groups(std::vector<int>& order, const std::vector<std::vector<int>>& deps, int n_ops, Same same,
                                    int gmax) {
  std::vector<int> leader(n_ops);
  for (int j = 0; j < n_ops; ++j) leader[j] = j;
  auto waits_for = [&](int y, int x) { return std::find(deps[y].begin(), deps[y].end(), x) != deps[y].end(); };
  for (size_t k = 0; k < order.size(); ++k) {
    const int x = order[k];
    if (leader[x] != x) continue;
    int members = 1;
    for (size_t q = k + 1; q < order.size() && q <= k + GROUP_LOOKAHEAD && members < gmax; ++q) {
      const int y = order[q];
      if (leader[y] != y || !same(x, y)) continue;
      // y may run at x's place when it waits for nothing from x (or x's followers) up to its own place.  (A path from one of
      // those ops to y ends in a direct edge from an op in this range: the order is topological.)
      bool free_ = true;
      for (size_t r = k; r < q && free_; ++r) free_ = !waits_for(y, order[r]);
      if (!free_) continue;
      leader[y] = x;
      order.erase(order.begin() + (long)q);
      order.insert(order.begin() + (long)(k + members), y);
      ++members;
    }
  }
  return leader;
}

// What must hold of a plan, checked on its own terms (tools/group_plan_check.cpp, tests): null, or the sentence that fails.
template <class Same>
inline const char* check_groups(const std::vector<int>& order, const std::vector<std::vector<int>>& deps,
                                const std::vector<int>& leader, const std::vector<int>& lane, Same same, int gmax) {
  const int n = (int)leader.size();
  std::vector<int> pos(n, -1), size(n, 0);
  for (size_t k = 0; k < order.size(); ++k) pos[order[k]] = (int)k;
  for (int j : order)
    for (int d : deps[j])
      if (pos[d] < 0 || pos[d] >= pos[j]) return "the enqueue order crosses a dependency edge";
  for (int j : order) {
    const int l = leader[j];
    if (l < 0 || l >= n || pos[l] < 0 || leader[l] != l) return "a follower's leader is no leader";
    ++size[l];
    if (l == j) continue;
    if (!same(l, j)) return "a group spans kernel instantiations";
    if (!lane.empty() && lane[l] != lane[j]) return "a group spans lanes";
    if (pos[j] <= pos[l] || pos[j] >= pos[l] + gmax) return "a group's ops are not adjacent in the enqueue order";
    for (int q = pos[l]; q < pos[j]; ++q) {
      if (leader[order[q]] != l) return "a group's ops are not adjacent in the enqueue order";
      if (std::find(deps[j].begin(), deps[j].end(), order[q]) != deps[j].end()) return "a group contains a dependency edge";
    }
  }
  for (int j : order)
    if (size[j] > gmax) return "a group is larger than the launch takes";
  return nullptr;
}

}  // namespace acrmi
