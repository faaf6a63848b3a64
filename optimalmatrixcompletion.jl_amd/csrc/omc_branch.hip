// omc_branch.hip -- the children of finished nodes by reference (omc_relax_append_children, omc_branch.h): k_branch_basis, one workgroup per
// distinct parent (the cut's v-hat and the candidate column of the row basis), and k_branch_write, one workgroup per child (the parent's
// descriptor copied into the child's rows of the per-node arrays, the new cut, its 2k + 1 rows and the column appended).
//
// The results are those of pack_nodes / put_descriptors (omc_api.cpp) bit for bit.  The host objects are built without fused multiply-adds
// and sum in index order, so here: no contraction (the pragma below holds for the whole file, cut_piece included), every sum of n terms on
// one lane in index order out of LDS, plain sqrt and / (correctly rounded for fp64).  Only the elementwise updates spread over the lanes.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#include "omc_branch.h"
#include "omc_cut_piece.h"

#define BRANCH_THREADS 256

// LDS: v (n doubles: x, then the candidate column), t (n doubles: the vector the running sum is taken against)
__global__ __launch_bounds__(BRANCH_THREADS) void k_branch_basis(const OmcWS w, const BranchWS b) {
  extern __shared__ double lds[];
  __shared__ double sh_d;
  __shared__ int sh_keep;
  const int p = blockIdx.x, tid = threadIdx.x, n = w.n, k = w.k;
  const size_t node = (size_t)b.slot_node[p];
  double* v = lds;
  double* t = lds + n;
  const double* x = w.obx + node * n;
  const double* Uh = w.oU + node * n * k;
  const double* Q = w.Qb + node * n * w.rmax;
  const int r = w.rr[node];
  for (int i = tid; i < n; i += BRANCH_THREADS) v[i] = x[i];
  // v-hat_j = sum_i Uhat[i, j] x[i]   (OMC.jl:1577)
  for (int j = 0; j < k; ++j) {
    __syncthreads();
    for (int i = tid; i < n; i += BRANCH_THREADS) t[i] = Uh[(size_t)j * n + i];
    __syncthreads();
    if (tid == 0) {
      double vh = 0.0;
      for (int i = 0; i < n; ++i) vh += t[i] * v[i];
      b.vhat[(size_t)p * k + j] = vh;
    }
  }
  // the candidate column x / ||x||: the row vector of the cut's first bound row (coefficient +1); ||x|| = 0 gives no column
  if (tid == 0) {
    double nx = 0.0;
    for (int i = 0; i < n; ++i) nx += v[i] * v[i];
    sh_d = sqrt(nx);
  }
  __syncthreads();
  const double nx = sh_d;
  if (!(nx > 0)) {      // the same for every lane
    if (tid == 0) b.keep[p] = 0;
    return;
  }
  for (int i = tid; i < n; i += BRANCH_THREADS) v[i] = v[i] / nx;
  // modified Gram-Schmidt, twice, against the parent's r columns
  for (int pass = 0; pass < 2; ++pass)
    for (int a = 0; a < r; ++a) {
      __syncthreads();      // v is complete, and every lane has read sh_d of the previous column
      for (int i = tid; i < n; i += BRANCH_THREADS) t[i] = Q[(size_t)a * n + i];
      __syncthreads();
      if (tid == 0) {
        double d = 0.0;
        for (int i = 0; i < n; ++i) d += t[i] * v[i];
        sh_d = d;
      }
      __syncthreads();
      const double d = sh_d;
      for (int i = tid; i < n; i += BRANCH_THREADS) v[i] -= d * t[i];
    }
  __syncthreads();
  if (tid == 0) {
    double nv = 0.0;
    for (int i = 0; i < n; ++i) nv += v[i] * v[i];
    nv = sqrt(nv);
    sh_d = nv;
    sh_keep = (nv > 1e-10 && r < n) ? 1 : 0;
    b.keep[p] = sh_keep;
  }
  __syncthreads();
  if (sh_keep) {
    const double nv = sh_d;
    for (int i = tid; i < n; i += BRANCH_THREADS) b.q[(size_t)p * n + i] = v[i] / nv;
  }
}

// Child c of the chunk is node first_child + c.  Every element of the child's strides is written: the parent's part, the new part, zero
// behind it (as put_descriptors does for the rows it uploads).
__global__ __launch_bounds__(BRANCH_THREADS) void k_branch_write(const OmcWS w, const BranchWS b, int first_child) {
  const int c = blockIdx.x, tid = threadIdx.x, n = w.n, k = w.k, Rm = w.Rmax, Lm = w.Lmax, rm = w.rmax;
  const int p = b.child_slot[c];
  const size_t par = (size_t)b.slot_node[p], ch = (size_t)first_child + c;
  const int Rp = w.R[par], Lp = b.slot_L[p], rp = w.rr[par], keep = b.keep[p];
  const int Rc = Rp + 2 * k + 1;
  // rows: the parent's, unchanged
  for (int e = tid; e < Rm; e += BRANCH_THREADS) {
    const bool in = e < Rp;
    w.rkind[ch * Rm + e] = in ? w.rkind[par * Rm + e] : 0;
    w.rcut[ch * Rm + e] = in ? w.rcut[par * Rm + e] : 0;
    w.rbi[ch * Rm + e] = in ? w.rbi[par * Rm + e] : 0;
    w.rbj[ch * Rm + e] = in ? w.rbj[par * Rm + e] : 0;
    w.rrhs[ch * Rm + e] = in ? w.rrhs[par * Rm + e] : 0.0;
  }
  for (int e = tid; e < Rm * k; e += BRANCH_THREADS) w.rcoef[(ch * Rm) * k + e] = e < Rp * k ? w.rcoef[(par * Rm) * k + e] : 0.0;
  // cuts: the parent's, then x
  const double* x = w.obx + par * n;
  for (int e = tid; e < Lm * n; e += BRANCH_THREADS) {
    const int l = e / n;
    w.cutx[ch * Lm * n + e] = l < Lp ? w.cutx[par * Lm * n + e] : (l == Lp ? x[e - l * n] : 0.0);
  }
  // row basis: the parent's columns, then q where x added one
  for (int e = tid; e < n * rm; e += BRANCH_THREADS) {
    const int a = e / n;
    w.Qb[ch * n * rm + e] = a < rp ? w.Qb[par * n * rm + e] : ((a == rp && keep) ? b.q[(size_t)p * n + (e - a * n)] : 0.0);
  }
  __syncthreads();      // the zeroes of the row arrays are down before one lane writes the new rows over them
  if (tid == 0) {
    // for every column j: v_j <= hi, -v_j <= -lo; then the cut row (OMC.jl:1680-1683), all with cut index Lp
    const int8_t* dr = b.dirs + (size_t)c * k;
    double icsum = 0.0;
    const size_t cut = ch * Rm + Rp + 2 * k;
    for (int j = 0; j < k; ++j) {
      double lo, hi, sl, ic;
      (void)cut_piece(b.cut_type, dr[j], b.vhat[(size_t)p * k + j], b.q1, &lo, &hi, &sl, &ic);      // the codes were checked on the host
      w.rcoef[cut * k + j] = -sl; icsum += ic;
      const size_t up = ch * Rm + Rp + 2 * j, dn = up + 1;
      w.rkind[up] = ROW_BOUND; w.rcut[up] = Lp; w.rbi[up] = -1; w.rbj[up] = j; w.rcoef[up * k + j] = 1.0; w.rrhs[up] = hi;
      w.rkind[dn] = ROW_BOUND; w.rcut[dn] = Lp; w.rbi[dn] = -1; w.rbj[dn] = j; w.rcoef[dn * k + j] = -1.0; w.rrhs[dn] = -lo;
    }
    w.rkind[cut] = ROW_CUT; w.rcut[cut] = Lp; w.rbi[cut] = -1; w.rbj[cut] = -1; w.rrhs[cut] = icsum;
    w.R[ch] = Rc; w.rr[ch] = rp + keep;
  }
}

extern "C" void omc_launch_branch(const OmcWS* w, const BranchWS* b, int nslots, int first_child, int nchildren, hipStream_t s) {
  hipLaunchKernelGGL(k_branch_basis, dim3(nslots), dim3(BRANCH_THREADS), 2 * sizeof(double) * (size_t)w->n, s, *w, *b);
  hipLaunchKernelGGL(k_branch_write, dim3(nchildren), dim3(BRANCH_THREADS), 0, s, *w, *b, first_child);
}
