// Runs the executor's grouping rule (csrc/group_plan.h) on a program read from standard input and holds the plan against the
// rule's own terms.  No GPU, no HIP (and so a program the host sanitizers can run):
//   c++ -std=c++17 -O1 tools/group_plan_check.cpp -o group_plan_check  &&  ./group_plan_check < program.txt
// Input: "n_ops n_bufs gmax", then per op, in program order, "key nR r.. nW w..": key = the kernel instantiation with a group
// form the op is routed to (0: none), the buffers it reads and the buffers it writes.
// Output: "groups N", one line "leader follower" per follower, the enqueue order on one line, then "ok" - or the sentence of the
// condition that does not hold, and exit status 1.  Lanes are not part of the input: a follower takes its leader's lane where the
// lanes are assigned (build_schedule), so a group cannot span two.
#include "../arbitrary-hands-3d-reconstruction_amd/csrc/group_plan.h"

#include <cstdio>

using namespace acrmi;

int main() {
  int n = 0, nb = 0, gmax = 0;
  if (std::scanf("%d %d %d", &n, &nb, &gmax) != 3 || n <= 0 || nb <= 0 || gmax < 1 || n > (1 << 20) || nb > (1 << 20)) {
    std::fprintf(stderr, "bad header\n");
    return 2;
  }
  std::vector<int> key(n), order(n);
  std::vector<std::vector<int>> reads(n), writes(n);
  for (int j = 0; j < n; ++j) {
    order[j] = j;
    int cnt = 0;
    if (std::scanf("%d %d", &key[j], &cnt) != 2 || cnt < 0 || cnt > nb) { std::fprintf(stderr, "bad op %d\n", j); return 2; }
    for (int pass = 0; pass < 2; ++pass) {
      std::vector<int>& v = pass ? writes[j] : reads[j];
      if (pass && (std::scanf("%d", &cnt) != 1 || cnt < 0 || cnt > nb)) { std::fprintf(stderr, "bad op %d\n", j); return 2; }
      v.resize(cnt);
      for (int& b : v)
        if (std::scanf("%d", &b) != 1 || b < 0 || b >= nb) { std::fprintf(stderr, "bad buffer in op %d\n", j); return 2; }
    }
  }
  const std::vector<std::vector<int>> deps = hazard_deps(order, reads, writes, n, nb);
  auto same = [&](int x, int y) { return key[x] != 0 && key[x] == key[y]; };
  const std::vector<int> leader = plan_groups(order, deps, n, same, gmax);
  int groups = 0;
  for (int j = 0; j < n; ++j) groups += leader[j] != j;
  std::printf("groups %d\n", groups);
  for (int j : order)
    if (leader[j] != j) std::printf("%d %d\n", leader[j], j);
  for (int j : order) std::printf("%d ", j);
  std::printf("\n");
  if (const char* why = check_groups(order, deps, leader, std::vector<int>(), same, gmax)) {
    std::printf("%s\n", why);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
