// omc_shor_index.h -- device builder of a Shor list's index structure (ShorGroupDev: mi, kid, cptr / cent, v1ptr / v1ent, v2ptr / v2ent,
// eclass, ctype, slackrow), DESIGN.md section 3.7a: descriptor, plan and launchers of omc_shor_index.hip.  Integer work only; the result is
// bit-identical to build_shor_group (omc_api.cpp).  The only synchronisation between workgroups is a kernel boundary.
#ifndef OMC_SHOR_INDEX_H
#define OMC_SHOR_INDEX_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SHIDX_TILE 1024      // items of one workgroup in a radix pass: four chunks of 256, ranked in item order
#define SHIDX_SCAN 1024      // elements of one workgroup in the scan

// error bits of meta[0]; the host reports them in this order (the order of build_shor_group)
#define SHIDX_ERR_RANGE 1
#define SHIDX_ERR_DUP 2
#define SHIDX_ERR_SOC 4

struct ShorIndexWS {
  int n, m, nq;
  int soc_fill;                    // 1: every entry is on the SOC list (n_soc = -1)
  const long long* idx;            // 4 nq: the wire tuples (1-based i1, i2, j1, j2)
  const long long* soc;            // 2 soc_cap: one chunk of the wire SOC pairs (1-based i, j)
  const uint8_t* mask;             // n m, column-major (the instance's)
  // scratch: two key / member buffers of 4 nq items, tile x digit counts, head flags, block sums of the scan
  unsigned long long *keyA, *keyB;
  unsigned *valA, *valB, *hist, *flag, *sums;
  // the structure, every array at its capacity (4nq, 4nq, nm+1, 4nq, 2nq+1, 2nq, 2nq+1, 2nq, m ; nm, m)
  int *mi, *kid, *cptr, *cent, *v1ptr, *v1ent, *v2ptr, *v2ent, *slackrow;
  uint8_t *eclass, *ctype;
  int* meta;                       // 4: error bits, nv1, nv2, 0
};

// What the shape fixes: radix passes of the four sorts (8-bit digits of the largest key the shape allows), scratch elements, launches.
struct ShorIndexPlan {
  int p_v1, p_v2, p_co, p_dup;
  long long items, tiles, hist, flag, sums;      // of the largest sort (4 nq items) ; head flags (2 nq + 1)
  long long launches;                            // kernels of one list, without the SOC scatter (one per chunk of explicit pairs)
};
static inline int shidx_passes(unsigned long long maxkey) {
  int bits = 0;
  while (maxkey) { ++bits; maxkey >>= 1; }
  return bits <= 8 ? 1 : (bits + 7) / 8;
}
static inline ShorIndexPlan shor_index_plan(long long n, long long m, long long nq) {
  ShorIndexPlan p;
  const bool any = n >= 2 && m >= 2;
  const unsigned long long un = (unsigned long long)n, um = (unsigned long long)m;
  const unsigned long long pair = any ? (un - 2) * un + (un - 1) : 0;      // (i1, i2) = (n - 2, n - 1)
  p.p_v1 = shidx_passes(any ? un * um * um - um - 1 : 0);                  // ((n-1) m + (m-2)) m + (m-1)
  p.p_v2 = shidx_passes(any ? pair * um + (um - 1) : 0);
  p.p_co = shidx_passes(any ? un * um - 1 : 0);
  p.p_dup = shidx_passes(any ? (pair * um + (um - 2)) * um + (um - 1) : 0);
  p.items = 4 * nq; p.tiles = (p.items + SHIDX_TILE - 1) / SHIDX_TILE; p.hist = 256 * p.tiles; p.flag = 2 * nq + 1;
  const long long scanned = p.hist > p.flag ? p.hist : p.flag;
  p.sums = (scanned + SHIDX_SCAN - 1) / SHIDX_SCAN + 1;
  // encode ; per pass: histogram, scan (3), scatter ; duplicate compare ; per V sort: keys, heads, scan (3), write ; coordinate keys ;
  // fill, cptr, columns.  An empty list: pointers, fill, cptr, columns.
  p.launches = nq > 0 ? 1 + 5ll * (p.p_dup + p.p_v1 + p.p_v2 + p.p_co) + 2 + 2 * 6 + 1 + 3 : 4;
  return p;
}

#ifdef __cplusplus
extern "C" {
#endif
// meta zeroed, tuples encoded and checked, the four sorts, heads / ids / pointers, eclass filled with 0 / 1.  Returns the kernels launched.
int omc_shidx_launch_sort(const ShorIndexWS* w, hipStream_t s);
// `count` explicit SOC pairs at w->soc: eclass = 1 there (between the two calls around it, once per chunk)
void omc_shidx_launch_soc(const ShorIndexWS* w, long long count, hipStream_t s);
// cptr, eclass = 2 on the minors' coordinates, ctype and slackrow.  Returns the kernels launched.
int omc_shidx_launch_finish(const ShorIndexWS* w, hipStream_t s);
#ifdef __cplusplus
}
#endif
#endif
