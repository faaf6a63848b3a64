// stand-alone host check of the pair arithmetic of k_setup_gram (omc_layout.h) under ASan + UBSan: every pair of every R is visited once,
// in row-major order of the upper triangle, by the chunks exactly as the kernel walks them
#include "omc_layout.h"
#include <cstdio>
#include <vector>
int main() {
  long checked = 0;
  for (int R = 1; R <= 300; ++R) {
    const int np = gram_npairs(R), nc = gram_chunks(R);
    std::vector<int> seen((size_t)R * R, 0);
    int er = 0, es = 0;      // expected pair in row-major order
    for (int c = 0; c < nc + 2; ++c) {      // two chunks beyond the end: the kernel's grid is sized by Rmax >= R
      int p = c * GRAM_CHUNK;
      if (p >= np) continue;
      const int pend = p + GRAM_CHUNK < np ? p + GRAM_CHUNK : np;
      int r, s; gram_pair_of(p, R, &r, &s);
      for (; p < pend; ++p) {
        if (r != er || s != es || r < 0 || s < r || s >= R) { printf("R %d p %d: (%d, %d), expected (%d, %d)\n", R, p, r, s, er, es); return 1; }
        seen[(size_t)r * R + s] += 1; ++checked;
        gram_pair_next(R, &r, &s);
        if (++es == R) { ++er; es = er; }
      }
    }
    for (int r = 0; r < R; ++r) for (int s = r; s < R; ++s) if (seen[(size_t)r * R + s] != 1) { printf("R %d: pair (%d, %d) seen %d times\n", R, r, s, seen[(size_t)r * R + s]); return 1; }
  }
  printf("ok: %ld pairs\n", checked);
  return 0;
}
