// What DensePlan::build makes of a tile adjacency: the features a linear-system test case is there to reach (tests/test_linear_ref.py).
//   plan_features n max_chains T  <T rows of T characters '0' / '1': the tile adjacency in natural order>
// prints one line of key=value pairs.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dense_plan.h"

using namespace bsg;

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: plan_features n max_chains T row...\n"); return 2; }
  const int n = std::atoi(argv[1]), max_chains = std::atoi(argv[2]), T = std::atoi(argv[3]);
  if (n <= 0 || T != (n + 63) / 64 || argc != 4 + T) { std::fprintf(stderr, "plan_features: %d rows of %d tiles expected\n", T, T); return 2; }
  std::vector<uint8_t> adj((size_t)T * T, 0);
  for (int i = 0; i < T; ++i) {
    if ((int)std::strlen(argv[4 + i]) != T) { std::fprintf(stderr, "plan_features: row %d is not %d long\n", i, T); return 2; }
    for (int j = 0; j < T; ++j) adj[(size_t)i * T + j] = argv[4 + i][j] == '1';
  }
  for (int i = 0; i < T; ++i) for (int j = 0; j < T; ++j) if (adj[(size_t)i * T + j] != adj[(size_t)j * T + i]) { std::fprintf(stderr, "plan_features: not symmetric\n"); return 2; }
  DensePlan P;
  P.build(n, adj, max_chains, 1, true);
  long chain = 0, ext = 0, split = 0, xilp = 0, xjchain = 0;
  for (const FusedTask& f : P.ftasks) {
    chain += (f.flags & kFusedChain) != 0;
    ext += (f.flags & kFusedExt) != 0;
    split += (f.flags & kFusedSplit) != 0;
    xilp += (f.flags & kFusedXiLp) != 0;
    xjchain += (f.flags & kFusedXjChain) != 0;
  }
  std::printf("n=%d T=%d max_chains=%d n_chains=%d panels=%zu tasks=%zu chain=%ld ext=%ld split=%ld xilp=%ld xjchain=%ld bs_level_sync=%d\n", n, T, max_chains,
              P.n_chains, P.panels.size(), P.ftasks.size(), chain, ext, split, xilp, xjchain, (int)P.bs_level_sync);
  return 0;
}
