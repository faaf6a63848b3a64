// omc_shor_cert.h -- device evaluator of caller-supplied Shor-mode multipliers (omc_shor_dual_bound_batch):
// descriptor and launchers of omc_shor_cert.hip.  A "view" is one evaluation: node view_node[v], with the blocks as given (view_way 0) or
// with their negative part removed first (view_way 1; sanitise = 1 evaluates both).  Nothing here touches a staged batch.
#ifndef OMC_SHOR_CERT_H
#define OMC_SHOR_CERT_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "omc_shor_relax.h"

#define SCERT_T 256

struct ShorCertWS {
  int n, m, B, V, nmb, nv1max, nv2max, clamp_zeta;      // nmb = minor blocks (SCERT_T minors each) per node at the call's stride
  long long nqs;                                        // nq_stride: stride of the per-minor planes
  double gamma;
  const ShorGroupDev* groups;
  const int *node_group, *view_node, *view_way;         // B ; V ; V
  const double* A; const uint8_t* mask;                 // n*m each, column-major (the instance's)
  const double *scale, *Gam, *zeta, *xi, *Xbar;         // B * (1, 15 nqs, m, n m, n m): the caller's multipliers
  double* GamC;                                         // B * 15 nqs: the blocks minus their negative part (NULL: not asked for)
  double* cleanpart;                                    // B * nmb: smallest eigenvalue of the blocks as given, per minor block
  double *e1, *e2;                                      // V * (nv1max, nv2max): mean residual per key
  double* row8;                                         // V * 8 nqs, SoA: Gamma'[0,p] (planes 0-3) and Gamma'[p,p] (planes 4-7), p = 1..4
  double* minpart;                                      // V * nmb * 2: sum of Gamma'[0,0] ; largest |residual| before the spread
  double *lamDX, *c0col, *colmu; int* colbad;           // V * (n m, m, m, m): dense multiplier, column constants, mu_j, 1 = mu <= 0 meets phi != 0, 2 = not finite
};

#ifdef __cplusplus
extern "C" {
#endif
void omc_scert_launch_clean(const ShorCertWS* w, int store, hipStream_t s);      /* one lane per minor of every node: defects, and GamC when store */
void omc_scert_launch_keys(const ShorCertWS* w, hipStream_t s);
void omc_scert_launch_minor(const ShorCertWS* w, hipStream_t s);
void omc_scert_launch_cols(const ShorCertWS* w, hipStream_t s);
#ifdef __cplusplus
}
#endif
#endif
