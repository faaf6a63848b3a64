// omc_cut_piece.h -- piece table of the disjunctive cuts (OMC.jl:1580-1678), once for the host (pack_nodes, omc_api.cpp; the dual-bound
// evaluators) and the device (k_branch_write, omc_branch.hip): lo <= v <= hi, g(v) = slope*v + icpt.  Plain arithmetic on one double, so
// both sides get the same bits; returns -1 for a direction code the cut type does not have.
#pragma once
#include <math.h>

#include "omc.h"

#ifdef __HIPCC__
#define OMC_CUT_HD __host__ __device__
#else
#define OMC_CUT_HD
#endif

static inline OMC_CUT_HD int cut_piece(int cut_type, int dir, double vhat, int q1, double* lo, double* hi, double* slope, double* icpt) {
  const double a = fabs(vhat);
  if (cut_type == OMC_CUT_LINEAR) {
    if (dir == OMC_DIR_LEFT) { *lo = -1; *hi = vhat; *slope = vhat - 1; *icpt = vhat; return 0; }      // 1582-1591
    if (dir == OMC_DIR_RIGHT) { *lo = vhat; *hi = 1; *slope = vhat + 1; *icpt = -vhat; return 0; }     // 1592-1601
  } else if (cut_type == OMC_CUT_LINEAR2) {
    if (dir == OMC_DIR_LEFT) { *lo = -1; *hi = -a; *slope = -(1 + a); *icpt = -a; return 0; }          // 1604-1613
    if (dir == OMC_DIR_MIDDLE) { *lo = -a; *hi = a; *slope = 0; *icpt = vhat * vhat; return 0; }       // 1614-1623
    if (dir == OMC_DIR_RIGHT) { *lo = a; *hi = 1; *slope = 1 + a; *icpt = -a; return 0; }              // 1624-1633
  } else if (cut_type == OMC_CUT_LINEAR3) {
    if (dir == OMC_DIR_LEFT) { *lo = -1; *hi = -a; *slope = -(1 + a); *icpt = -a; return 0; }          // 1636-1645
    if (dir == OMC_DIR_INNER_LEFT) { *lo = -a; *hi = 0; *slope = -a; *icpt = 0; return 0; }            // 1646-1655
    if (dir == OMC_DIR_INNER_RIGHT) { *lo = 0; *hi = a; *slope = a; *icpt = 0; return 0; }             // 1656-1665
    if (dir == OMC_DIR_RIGHT) {                                                                        // 1666-1675
      *lo = a; *hi = 1;
      if (q1) { *slope = a; *icpt = 0; } else { *slope = 1 + a; *icpt = -a; }
      return 0;
    }
  }
  return -1;
}
