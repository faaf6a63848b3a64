// omc_shor_index.hip -- a Shor list's index structure built on the device (omc_shor_index.h).
//
// One list at a time, as a fixed sequence of launches on one stream (the sequence follows from (n, m, nq) alone):
//   k_shidx_encode     one thread per minor: range test of build_shor_group, mi (SoA)
//   k_shidx_keys       the items of one sort in member order: duplicate key, V1 keys, V2 keys or coordinate ids
//   radix pass (x passes of the shape's largest key): k_shidx_hist (tile x digit counts in LDS), scan, k_shidx_scatter (stable: ranks in item
//                      order by wave ballots and a per-wave digit prefix in LDS).  Items start in member order, so the stable sort on the key
//                      alone gives the host's (key, member) order.
//   k_shidx_dup        adjacent compare of the sorted duplicate keys
//   k_shidx_heads, scan, k_shidx_vwrite     segment heads -> key ids, v?ptr, kid (scattered back through the member), nv
//   k_shidx_fill, k_shidx_soc, k_shidx_cptr, k_shidx_cols     eclass, cptr (lower bound per coordinate in the sorted ids), ctype / slackrow
// Workgroups meet at kernel boundaries only.  Integer atomics where the result does not depend on arrival order (LDS digit counts, the
// error bits); every array is the same from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "omc_shor_index.h"

typedef unsigned long long u64;
typedef unsigned u32;

namespace {

__global__ __launch_bounds__(256) void k_shidx_encode(ShorIndexWS w) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= w.nq) return;
  const long long* t = w.idx + 4 * (size_t)q;
  long long i1 = t[0] - 1, i2 = t[1] - 1, j1 = t[2] - 1, j2 = t[3] - 1;
  if (!(0 <= i1 && i1 < i2 && i2 < w.n && 0 <= j1 && j1 < j2 && j2 < w.m)) {
    atomicOr(w.meta, SHIDX_ERR_RANGE);
    i1 = i2 = j1 = j2 = 0;      // the list is refused; every later index stays in range
  }
  const size_t nq = (size_t)w.nq;
  w.mi[q] = (int)i1; w.mi[nq + q] = (int)i2; w.mi[2 * nq + q] = (int)j1; w.mi[3 * nq + q] = (int)j2;
}

// kind 0: duplicate key of minor e ; 1: V1 key of member e = 2 q + which ; 2: V2 key of member e = 2 q + which ; 3: coordinate id of member
// e = 4 q + p, p in block order (i1,j1), (i1,j2), (i2,j1), (i2,j2)
__global__ __launch_bounds__(256) void k_shidx_keys(ShorIndexWS w, int kind, u32 N) {
  const u32 e = blockIdx.x * 256u + threadIdx.x;
  if (e >= N) return;
  const size_t nq = (size_t)w.nq;
  const u32 q = kind == 0 ? e : (kind == 3 ? e >> 2 : e >> 1), p = kind == 3 ? (e & 3u) : (e & 1u);
  const u64 i1 = (u64)w.mi[q], i2 = (u64)w.mi[nq + q], j1 = (u64)w.mi[2 * nq + q], j2 = (u64)w.mi[3 * nq + q];
  const u64 n = (u64)w.n, m = (u64)w.m;
  u64 key;
  if (kind == 0) key = ((i1 * n + i2) * m + j1) * m + j2;
  else if (kind == 1) key = ((p ? i2 : i1) * m + j1) * m + j2;
  else if (kind == 2) key = (i1 * n + i2) * m + (p ? j2 : j1);
  else key = ((p & 1u) ? j2 : j1) * n + ((p & 2u) ? i2 : i1);
  w.keyA[e] = key;
  if (kind != 0) w.valA[e] = e;
}

// counts of one tile per digit, digit-major: the scan over the whole array gives every (digit, tile) its first output position
__global__ __launch_bounds__(256) void k_shidx_hist(const u64* __restrict__ keys, u32 N, int shift, u32* __restrict__ hist, u32 ntiles) {
  __shared__ u32 h[256];
  const u32 tid = threadIdx.x, tile = blockIdx.x;
  h[tid] = 0;
  __syncthreads();
  for (u32 c = 0; c < SHIDX_TILE / 256; ++c) {
    const u32 e = tile * SHIDX_TILE + c * 256u + tid;
    if (e < N) atomicAdd(&h[(u32)(keys[e] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(size_t)tid * ntiles + tile] = h[tid];
}

__global__ __launch_bounds__(256) void k_shidx_scatter(const u64* __restrict__ kin, const u32* __restrict__ vin, u64* __restrict__ kout,
                                                        u32* __restrict__ vout, u32 N, int shift, const u32* __restrict__ hist, u32 ntiles) {
  __shared__ u32 base[256];
  __shared__ u32 wc[4][256];
  const u32 tid = threadIdx.x, tile = blockIdx.x, wave = tid >> 6, lane = tid & 63u;
  base[tid] = hist[(size_t)tid * ntiles + tile];
  for (u32 c = 0; c < SHIDX_TILE / 256; ++c) {
    wc[0][tid] = 0; wc[1][tid] = 0; wc[2][tid] = 0; wc[3][tid] = 0;
    __syncthreads();
    const u32 e = tile * SHIDX_TILE + c * 256u + tid;
    const bool valid = e < N;
    const u64 key = valid ? kin[e] : 0ull;
    const u32 d = (u32)(key >> shift) & 255u;
    // lanes of this wave with the same digit (invalid lanes form no group)
    u64 same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const u64 bal = __ballot(valid && bit);
      same &= bit ? bal : ~bal;
    }
    const u32 rank = (u32)__popcll(same & ((1ull << lane) - 1ull));
    if (valid && rank == 0) wc[wave][d] = (u32)__popcll(same);
    __syncthreads();
    if (valid) {
      u32 pos = base[d] + rank;
      for (u32 w2 = 0; w2 < wave; ++w2) pos += wc[w2][d];
      kout[pos] = key;
      if (vin) vout[pos] = vin[e];
    }
    __syncthreads();
    base[tid] += wc[0][tid] + wc[1][tid] + wc[2][tid] + wc[3][tid];
    __syncthreads();
  }
}

// ---- exclusive scan of M unsigned counts in place: block sums, the sums by one workgroup, the blocks again ------------------------------------
__device__ __forceinline__ u32 block_incl_scan(u32 v, u32* sh, u32 tid) {
  sh[tid] = v;
  __syncthreads();
  for (u32 off = 1; off < 256; off <<= 1) {
    const u32 t = tid >= off ? sh[tid - off] : 0u;
    __syncthreads();
    sh[tid] += t;
    __syncthreads();
  }
  return sh[tid];
}
__global__ __launch_bounds__(256) void k_shidx_scan_sums(const u32* __restrict__ a, u32 M, u32* __restrict__ sums) {
  __shared__ u32 sh[256];
  const u32 tid = threadIdx.x, e0 = blockIdx.x * SHIDX_SCAN + tid * 4u;
  u32 t = 0;
  for (u32 r = 0; r < 4; ++r) if (e0 + r < M) t += a[e0 + r];
  const u32 incl = block_incl_scan(t, sh, tid);
  if (tid == 255) sums[blockIdx.x] = incl;
}
__global__ __launch_bounds__(256) void k_shidx_scan_top(u32* __restrict__ sums, u32 nb) {
  __shared__ u32 sh[256];
  const u32 tid = threadIdx.x;
  u32 carry = 0;
  for (u32 b0 = 0; b0 < nb; b0 += 256) {
    const u32 v = b0 + tid < nb ? sums[b0 + tid] : 0u;
    const u32 incl = block_incl_scan(v, sh, tid);
    if (b0 + tid < nb) sums[b0 + tid] = carry + incl - v;
    carry += sh[255];
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void k_shidx_scan_apply(u32* __restrict__ a, u32 M, const u32* __restrict__ sums) {
  __shared__ u32 sh[256];
  const u32 tid = threadIdx.x, e0 = blockIdx.x * SHIDX_SCAN + tid * 4u;
  u32 v[4], t = 0;
  for (u32 r = 0; r < 4; ++r) { v[r] = e0 + r < M ? a[e0 + r] : 0u; t += v[r]; }
  u32 run = sums[blockIdx.x] + block_incl_scan(t, sh, tid) - t;
  for (u32 r = 0; r < 4; ++r) { if (e0 + r < M) a[e0 + r] = run; run += v[r]; }
}

__global__ __launch_bounds__(256) void k_shidx_dup(const u64* __restrict__ keys, u32 N, int* meta) {
  const u32 e = blockIdx.x * 256u + threadIdx.x;
  if (e >= 1 && e < N && keys[e] == keys[e - 1]) atomicOr(meta, SHIDX_ERR_DUP);
}

// flag[e] = 1 at the first item of a key, e = 0..N-1 ; flag[N] = 0, so that the exclusive scan leaves the number of keys there
__global__ __launch_bounds__(256) void k_shidx_heads(const u64* __restrict__ keys, u32 N, u32* __restrict__ flag) {
  const u32 e = blockIdx.x * 256u + threadIdx.x;
  if (e > N) return;
  flag[e] = (e < N && (e == 0 || keys[e] != keys[e - 1])) ? 1u : 0u;
}
// heads[e] = keys before item e (scanned flags).  ent holds the sorted members already (the last scatter wrote them there).
__global__ __launch_bounds__(256) void k_shidx_vwrite(const u32* __restrict__ heads, const int* __restrict__ ent, u32 N, u32 nq, int* __restrict__ ptr,
                                                       int* __restrict__ kid, int* nv_out) {
  const u32 e = blockIdx.x * 256u + threadIdx.x;
  if (e > N) return;
  if (e == N) { ptr[heads[N]] = (int)N; *nv_out = (int)heads[N]; return; }
  const u32 id = heads[e + 1] - 1u;
  if (heads[e + 1] != heads[e]) ptr[id] = (int)e;
  const u32 member = (u32)ent[e];
  kid[(size_t)(member & 1u) * nq + (member >> 1)] = (int)id;
}
__global__ void k_shidx_empty(ShorIndexWS w) { w.v1ptr[0] = 0; w.v2ptr[0] = 0; }

__global__ __launch_bounds__(256) void k_shidx_fill(uint8_t* __restrict__ eclass, u32 nm, uint8_t v) {
  const u32 e = blockIdx.x * 256u + threadIdx.x;
  if (e < nm) eclass[e] = v;
}
__global__ __launch_bounds__(256) void k_shidx_soc(ShorIndexWS w, long long count) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= count) return;
  const long long i = w.soc[2 * c] - 1, j = w.soc[2 * c + 1] - 1;
  if (!(0 <= i && i < w.n && 0 <= j && j < w.m)) { atomicOr(w.meta, SHIDX_ERR_SOC); return; }
  w.eclass[(size_t)j * w.n + i] = 1;
}
// cptr[e] = first position of coordinate e in the sorted ids (e = 0..nm) ; a coordinate that occurs is of class 2
__global__ __launch_bounds__(256) void k_shidx_cptr(ShorIndexWS w, const u64* __restrict__ ids, u32 N) {
  const u32 e = blockIdx.x * 256u + threadIdx.x, nm = (u32)w.n * (u32)w.m;
  if (e > nm) return;
  u32 lo = 0, hi = N;
  while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (ids[mid] < (u64)e) lo = mid + 1; else hi = mid; }
  w.cptr[e] = (int)lo;
  if (e < nm && lo < N && ids[lo] == (u64)e) w.eclass[e] = 2;
}
// one wave per column: first row outside the minors' coordinates, first unobserved one among them (64 rows per ballot)
__global__ __launch_bounds__(256) void k_shidx_cols(ShorIndexWS w) {
  const int j = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= w.m) return;
  const int n = w.n;
  int first_nonC = -1, first_unobs = -1;
  for (int i0 = 0; i0 < n && first_unobs < 0; i0 += 64) {
    const int i = i0 + lane;
    const bool in = i < n;
    const bool nonC = in && w.eclass[(size_t)j * n + i] != 2;
    const bool unobs = nonC && !w.mask[(size_t)j * n + i];
    const u64 b1 = __ballot(nonC), b2 = __ballot(unobs);
    if (first_nonC < 0 && b1) first_nonC = i0 + __ffsll((long long)b1) - 1;
    if (b2) first_unobs = i0 + __ffsll((long long)b2) - 1;
  }
  if (lane == 0) {
    if (first_unobs >= 0) { w.ctype[j] = 0; w.slackrow[j] = first_unobs; }
    else if (first_nonC >= 0) { w.ctype[j] = 1; w.slackrow[j] = first_nonC; }
    else { w.ctype[j] = 2; w.slackrow[j] = -1; }
  }
}

static inline u32 blocks(u64 count, u32 per) { return (u32)((count + per - 1) / per > 0 ? (count + per - 1) / per : 1); }

static int scan_counts(const ShorIndexWS* w, u32* a, u32 M, hipStream_t s) {
  const u32 nb = blocks(M, SHIDX_SCAN);
  hipLaunchKernelGGL(k_shidx_scan_sums, dim3(nb), dim3(256), 0, s, a, M, w->sums);
  hipLaunchKernelGGL(k_shidx_scan_top, dim3(1), dim3(256), 0, s, w->sums, nb);
  hipLaunchKernelGGL(k_shidx_scan_apply, dim3(nb), dim3(256), 0, s, a, M, w->sums);
  return 3;
}
// `passes` stable passes over the items of keyA / valA ; the sorted keys end in *sorted, the sorted members in final_vals (NULL: no payload)
static int radix_sort(const ShorIndexWS* w, u32 N, int passes, u32* final_vals, const u64** sorted, hipStream_t s) {
  u64 *kin = w->keyA, *kout = w->keyB;
  u32 *vin = w->valA, *vout = w->valB;
  const u32 ntiles = blocks(N, SHIDX_TILE);
  int launches = 0;
  for (int p = 0; p < passes; ++p) {
    u32* vdst = p == passes - 1 ? final_vals : vout;
    hipLaunchKernelGGL(k_shidx_hist, dim3(ntiles), dim3(256), 0, s, kin, N, 8 * p, w->hist, ntiles);
    launches += 1 + scan_counts(w, w->hist, 256u * ntiles, s);
    hipLaunchKernelGGL(k_shidx_scatter, dim3(ntiles), dim3(256), 0, s, kin, final_vals ? vin : (const u32*)nullptr, kout, vdst, N, 8 * p, w->hist, ntiles);
    ++launches;
    u64* tk = kin; kin = kout; kout = tk;
    u32* tv = vin; vin = vout; vout = tv;
  }
  *sorted = kin;
  return launches;
}
static int v_keys(const ShorIndexWS* w, int kind, int passes, int* ptr, int* ent, int* kid, int* nv_out, hipStream_t s) {
  const u32 N = 2u * (u32)w->nq;
  const u64* sorted = nullptr;
  hipLaunchKernelGGL(k_shidx_keys, dim3(blocks(N, 256)), dim3(256), 0, s, *w, kind, N);
  int launches = 1 + radix_sort(w, N, passes, (u32*)ent, &sorted, s);
  hipLaunchKernelGGL(k_shidx_heads, dim3(blocks((u64)N + 1, 256)), dim3(256), 0, s, sorted, N, w->flag);
  launches += 1 + scan_counts(w, w->flag, N + 1, s);
  hipLaunchKernelGGL(k_shidx_vwrite, dim3(blocks((u64)N + 1, 256)), dim3(256), 0, s, w->flag, ent, N, (u32)w->nq, ptr, kid, nv_out);
  return launches + 1;
}

}  // namespace

extern "C" int omc_shidx_launch_sort(const ShorIndexWS* w, hipStream_t s) {
  const ShorIndexPlan P = shor_index_plan(w->n, w->m, w->nq);
  const u32 nq = (u32)w->nq, nm = (u32)w->n * (u32)w->m;
  int launches = 0;
  (void)hipMemsetAsync(w->meta, 0, 4 * sizeof(int), s);
  if (nq > 0) {
    const u64* sorted = nullptr;
    hipLaunchKernelGGL(k_shidx_encode, dim3(blocks(nq, 256)), dim3(256), 0, s, *w);
    hipLaunchKernelGGL(k_shidx_keys, dim3(blocks(nq, 256)), dim3(256), 0, s, *w, 0, nq);
    launches += 2 + radix_sort(w, nq, P.p_dup, nullptr, &sorted, s);
    hipLaunchKernelGGL(k_shidx_dup, dim3(blocks(nq, 256)), dim3(256), 0, s, sorted, nq, w->meta);
    ++launches;
    launches += v_keys(w, 1, P.p_v1, w->v1ptr, w->v1ent, w->kid, w->meta + 1, s);
    launches += v_keys(w, 2, P.p_v2, w->v2ptr, w->v2ent, w->kid + 2 * (size_t)nq, w->meta + 2, s);
  } else {
    hipLaunchKernelGGL(k_shidx_empty, dim3(1), dim3(1), 0, s, *w);
    ++launches;
  }
  hipLaunchKernelGGL(k_shidx_fill, dim3(blocks(nm, 256)), dim3(256), 0, s, w->eclass, nm, (uint8_t)(w->soc_fill ? 1 : 0));
  return launches + 1;
}

extern "C" void omc_shidx_launch_soc(const ShorIndexWS* w, long long count, hipStream_t s) {
  if (count > 0) hipLaunchKernelGGL(k_shidx_soc, dim3(blocks((u64)count, 256)), dim3(256), 0, s, *w, count);
}

extern "C" int omc_shidx_launch_finish(const ShorIndexWS* w, hipStream_t s) {
  const ShorIndexPlan P = shor_index_plan(w->n, w->m, w->nq);
  const u32 N = 4u * (u32)w->nq, nm = (u32)w->n * (u32)w->m;
  int launches = 0;
  const u64* sorted = w->keyA;      // an empty list: no id is read
  if (N > 0) {
    hipLaunchKernelGGL(k_shidx_keys, dim3(blocks(N, 256)), dim3(256), 0, s, *w, 3, N);
    launches += 1 + radix_sort(w, N, P.p_co, (u32*)w->cent, &sorted, s);
  }
  hipLaunchKernelGGL(k_shidx_cptr, dim3(blocks((u64)nm + 1, 256)), dim3(256), 0, s, *w, sorted, N);
  hipLaunchKernelGGL(k_shidx_cols, dim3(blocks((u64)w->m, 4)), dim3(256), 0, s, *w);
  return launches + 2;
}
