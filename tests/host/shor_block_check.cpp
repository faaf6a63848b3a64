// Stand-alone host program around csrc/omc_shor_block.h (tests/test_shor_block_cpu.py): nothing of the project but that header.
// stdin: the number of blocks, then per block the 15 packed entries and the four key residuals e12, e34, e13, e24.
// stdout, per block, one line of %.17g values: the smallest eigenvalue of the block as given | the block minus its negative part (15) |
// the block as given after the spread, Gamma - E + ||E||_F I (15) | ||E||_F | the final shift | the block after the final shift (15).
#include <cstdio>
#include <vector>
#include "omc_shor_block.h"

static void put(const double* g, int count) {
  for (int e = 0; e < count; ++e) std::printf(" %.17g", g[e]);
}

int main() {
  int nblocks = 0;
  if (std::scanf("%d", &nblocks) != 1 || nblocks < 0) return 2;
  std::vector<double> in(19);
  for (int b = 0; b < nblocks; ++b) {
    for (int e = 0; e < 19; ++e)
      if (std::scanf("%lf", &in[e]) != 1) return 3;
    double clean[15], g[15];
    for (int e = 0; e < 15; ++e) { clean[e] = in[e]; g[e] = in[e]; }
    const double lo = shor_block_min_eig(in.data());
    (void)shor_block_remove_negative(clean);
    if (!shor_block_finite(g)) return 4;
    std::printf("%.17g", lo);
    put(clean, 15);
    const double nrm = shor_block_spread(g, in[15], in[16], in[17], in[18], shor_block_e3(g));
    put(g, 15);
    const double sh = shor_block_final_shift(g);
    std::printf(" %.17g %.17g", nrm, sh);
    put(g, 15);
    std::printf("\n");
  }
  return 0;
}
