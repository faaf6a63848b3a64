// omc_api_minors.cpp -- enumeration and selection of Shor minors behind the C ABI of include/omc.h: omc_shor_count, omc_shor_indexes,
// omc_violated_shor_minors, omc_shor_last_stats, omc_shor_last_select_stats.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <string>
#include <vector>

#include "omc_api_internal.h"

#include "omc_shor.h"

// ---------------------------------------------------------------------------------------------------------------------
// Shor minors: generate_rank1_matrix_completion_Shor_constraints_indexes (OMC.jl:2545-2612) and
// generate_violated_Shor_minors (OMC.jl:2614-2640).  Kernels in omc_shor.hip; the host only sequences the segments.
// ---------------------------------------------------------------------------------------------------------------------
struct ShorSeg { int kind, la, lb; };
static void shor_segments(int n_classes, const int* classes, bool dedup, std::vector<ShorSeg>& segs) {
  bool seen[5] = {false, false, false, false, false};
  for (int c = 0; c < n_classes; ++c) {
    const int p = classes[c];
    if (p < 0 || p > 4) continue;                 // the reference's if/elseif chain has no branch for other values
    if (dedup) { if (seen[p]) continue; seen[p] = true; }
    if (p == 4) segs.push_back({SH_COMBO, SH_BOTH, 0});                                       // OMC.jl:2556-2561
    else if (p == 3) segs.push_back({SH_PRODUCT, SH_BOTH, SH_XOR});                           // 2562-2569
    else if (p == 2) { segs.push_back({SH_PRODUCT, SH_BOTH, SH_NONE}); segs.push_back({SH_COMBO, SH_XOR, 0}); }  // 2570-2584
    else if (p == 1) segs.push_back({SH_PRODUCT, SH_XOR, SH_NONE});                           // 2585-2596
    else segs.push_back({SH_COMBO, SH_NONE, 0});                                              // 2597-2608
  }
}
static int shor_prepare(omc_instance* h) {
  if (h->shor_ready) return 0;
  const int n = h->n, m = h->m;
  if (m > 8192) return fail(OMC_ERR_UNSUPPORTED, "Shor enumeration supports m <= 8192 in this build");
  HIPCHK(hipSetDevice(h->device));
  const int W = (m + 63) / 64;
  std::vector<uint64_t> bits((size_t)n * W, 0);
  for (int j = 0; j < m; ++j)
    for (int i = 0; i < n; ++i)
      if (h->mask[(size_t)j * n + i]) bits[(size_t)i * W + (j >> 6)] |= (1ULL << (j & 63));
  const long long np = (long long)n * (n - 1) / 2;
  int rc;
  if ((rc = upload(h->sbits, bits.data(), bits.size() * 8, h->stream))) return rc;
  if ((rc = h->scb.ensure((size_t)std::max(np, 1LL) * 4)) || (rc = h->scx.ensure((size_t)std::max(np, 1LL) * 4)) ||
      (rc = h->scz.ensure((size_t)std::max(np, 1LL) * 4)) || (rc = h->soff.ensure((size_t)std::max(np, 1LL) * 8)) ||
      (rc = h->stot.ensure(64)) || (rc = h->shist.ensure(256 * 8)) || (rc = h->scnt.ensure(64)))
    return rc;
  omc_shor_launch_pair_counts(n, m, W, h->sbits.as<uint64_t>(), np, h->scb.as<int>(), h->scx.as<int>(), h->scz.as<int>(), h->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));   // `bits` is a host temporary
  h->shor_W = W; h->shor_pairs = np; h->shor_ready = true;
  return 0;
}
// scan segment `sg` with offsets starting at `base`; returns its total
static int shor_scan(omc_instance* h, const ShorSeg& sg, long long base, long long* total) {
  omc_shor_launch_seg_scan(sg.kind, sg.la, sg.lb, h->scb.as<int>(), h->scx.as<int>(), h->scz.as<int>(), h->shor_pairs, base,
                           h->soff.as<long long>(), h->stot.as<long long>(), h->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(total, h->stot.p, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int omc_shor_count(omc_instance* h, int n_classes, const int* num_entries_present, int64_t* count_per_class) {
  if (!h || (n_classes > 0 && !num_entries_present) || !count_per_class) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  int rc = shor_prepare(h);
  if (rc) return rc;
  for (int c = 0; c < n_classes; ++c) {
    std::vector<ShorSeg> segs;
    shor_segments(1, num_entries_present + c, false, segs);
    long long tot = 0;
    for (const ShorSeg& sg : segs) { long long t = 0; if ((rc = shor_scan(h, sg, 0, &t))) return rc; tot += t; }
    count_per_class[c] = tot;
  }
  return 0;
}

int omc_shor_indexes(omc_instance* h, int n_classes, const int* num_entries_present, int64_t capacity, int64_t* out, int64_t* count) {
  if (!h || (n_classes > 0 && !num_entries_present) || !count) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  int rc = shor_prepare(h);
  if (rc) return rc;
  std::vector<ShorSeg> segs;
  shor_segments(n_classes, num_entries_present, false, segs);
  std::vector<long long> tot(segs.size(), 0);
  long long total = 0;
  for (size_t q = 0; q < segs.size(); ++q) { if ((rc = shor_scan(h, segs[q], 0, &tot[q]))) return rc; total += tot[q]; }
  *count = total;
  if (!out || capacity < total || total == 0) return 0;      // size query (or nothing to write)
  if ((rc = h->sout.ensure((size_t)total * 32))) return rc;
  EventPair ev;
  if (ev.create()) return fail(999, "hipEventCreate failed");
  hipEvent_t e0 = ev.e0, e1 = ev.e1;
  HIPCHK(hipEventRecord(e0, h->stream));
  long long base = 0;
  for (size_t q = 0; q < segs.size(); ++q) {
    long long t = 0;
    if ((rc = shor_scan(h, segs[q], base, &t))) return rc;
    omc_shor_launch_enum_tuples(h->n, h->m, h->shor_W, h->sbits.as<uint64_t>(), segs[q].kind, segs[q].la, segs[q].lb,
                                h->soff.as<long long>(), h->shor_pairs, h->sout.as<long long>(), h->stream);
    HIPCHK(hipGetLastError());
    base += t;
  }
  HIPCHK(hipEventRecord(e1, h->stream));
  HIPCHK(hipMemcpyAsync(out, h->sout.p, (size_t)total * 32, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  float ms = 0; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  h->shor_last_ms = ms; h->shor_last_candidates = total;
  return 0;
}

// MSD radix select of the K largest of the N 128-bit keys (hi, lo), 1 <= K <= N: finds a digit prefix (*bhi, *blo) such that the keys >= it are
// the K largest and at most SHOR_SEL_CAP more, and emits those to sohi / solo (*got of them, in no particular order)
static const long long SHOR_SEL_CAP = 8192;
static int shor_select_emit(omc_instance* h, long long N, long long K, uint64_t* bhi, uint64_t* blo, unsigned long long* got) {
  uint64_t phi = 0, plo = 0; long long need = K; unsigned long long bin = 0;
  for (int level = 0; level < 16; ++level) {
    HIPCHK(hipMemsetAsync(h->shist.p, 0, 256 * 8, h->stream));
    omc_shor_launch_hist(N, h->shi.as<uint64_t>(), h->slo.as<uint64_t>(), phi, plo, level, h->shist.as<unsigned long long>(), h->stream);
    HIPCHK(hipGetLastError());
    unsigned long long hist[256];
    HIPCHK(hipMemcpyAsync(hist, h->shist.p, sizeof(hist), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    long long cum = 0; int d = 255;
    for (; d > 0; --d) { if (cum + (long long)hist[d] >= need) break; cum += (long long)hist[d]; }
    need -= cum; bin = hist[d];
    if (level < 8) phi |= (uint64_t)d << (56 - 8 * level); else plo |= (uint64_t)d << (56 - 8 * (level - 8));
    if ((long long)bin - need <= SHOR_SEL_CAP) break;
  }
  const unsigned long long cap = (unsigned long long)(K + SHOR_SEL_CAP + 16);
  int rc;
  if ((rc = h->sohi.ensure(cap * 8)) || (rc = h->solo.ensure(cap * 8))) return rc;
  HIPCHK(hipMemsetAsync((char*)h->scnt.p + 8, 0, 8, h->stream));
  omc_shor_launch_emit(N, h->shi.as<uint64_t>(), h->slo.as<uint64_t>(), phi, plo, h->sohi.as<uint64_t>(), h->solo.as<uint64_t>(),
                       h->scnt.as<unsigned long long>() + 1, cap, h->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(got, (char*)h->scnt.p + 8, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (*got > cap || (long long)*got < K) return fail(OMC_ERR_ARGUMENT, "internal: radix select emitted an unexpected number of keys");
  *bhi = phi; *blo = plo;
  return 0;
}

// Streaming selection: the K largest keys without the key of every candidate in memory.  The segments are walked in tiles of
// consecutive row pairs; the enumerator keeps the candidates at or above the threshold in a buffer of `capacity` keys (shi / slo), and
// whenever enough new keys have arrived the radix select above reduces it to the K largest (+ at most SHOR_SEL_CAP) and its boundary becomes the
// threshold.  Keys are unique, so the K largest are a unique set whatever the tiles and the order of the appends; on return they are in
// sohi / solo (*got of them) exactly as the materialised path leaves them.
//   capacity = max(budget / 16, K + SHOR_SEL_CAP + largest candidate count of one row pair in one segment): after a compaction at most
//   K + SHOR_SEL_CAP keys remain, so a tile of one pair always fits and the walk terminates for any budget.
static int shor_stream_select(omc_instance* h, const std::vector<ShorSeg>& segs, long long n_existing_keys, long long K, long long budget_bytes,
                              unsigned long long* got) {
  const int n = h->n, m = h->m, k = h->k;
  const long long np = h->shor_pairs;
  int rc;
  // per-pair offsets of every segment on the host (off[np] = the segment's total)
  std::vector<std::vector<long long>> hoff(segs.size());
  long long maxpair = 0;
  for (size_t q = 0; q < segs.size(); ++q) {
    hoff[q].resize((size_t)np + 1);
    if ((rc = shor_scan(h, segs[q], 0, &hoff[q][(size_t)np]))) return rc;
    HIPCHK(hipMemcpyAsync(hoff[q].data(), h->soff.p, (size_t)np * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (long long t = 0; t < np; ++t) maxpair = std::max(maxpair, hoff[q][(size_t)t + 1] - hoff[q][(size_t)t]);
  }
  const long long nominal = std::max<long long>(budget_bytes / 16, 1);      // the buffer the budget asks for; tiles and compactions are paced by it
  const long long capacity = std::max(nominal, K + SHOR_SEL_CAP + maxpair);
  if ((rc = h->shi.ensure((size_t)capacity * 8)) || (rc = h->slo.ensure((size_t)capacity * 8))) return rc;
  h->shor_sel[3] = 16 * capacity;
  unsigned long long* d_count = h->scnt.as<unsigned long long>() + 2;       // survivor counter; the overflow flag is the word after it
  unsigned int* d_flag = (unsigned int*)(h->scnt.as<unsigned long long>() + 3);
  uint64_t thi = 0, tlo = 0;                                                 // every key is >= (0, 1): the first tiles keep every candidate
  long long count = 0, compacted_at = 0;
  auto set_count = [&](long long c) -> int {
    const unsigned long long w[2] = {(unsigned long long)c, 0ULL};
    HIPCHK(hipMemcpyAsync(d_count, w, 16, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));                                 // `w` is a stack temporary
    return 0;
  };
  auto compact = [&]() -> int {                                              // count > K
    unsigned long long g = 0;
    int r = shor_select_emit(h, count, K, &thi, &tlo, &g);
    if (r) return r;
    HIPCHK(hipMemcpyAsync(h->shi.p, h->sohi.p, g * 8, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->slo.p, h->solo.p, g * 8, hipMemcpyDeviceToDevice, h->stream));
    count = compacted_at = (long long)g;
    ++h->shor_sel[2];
    return set_count(count);
  };
  if ((rc = set_count(0))) return rc;
  const long long TILE_MAX = 1LL << 32;      // candidates: ~0.1 s of the scorer, so the host looks at the counter often enough
  double gain = 1.0;                         // candidates per free slot that the last tile's survival rate allows (half the free space filled)
  // while most candidates survive (no threshold yet, or scores that grow along the enumeration) a tile can only fill the buffer: such tiles start
  // at 1/64 of the budget, so that the first threshold costs a small select, and double as long as that goes on
  long long probe = std::min(nominal, std::max(nominal / 64, 65536LL));
  for (size_t q = 0; q < segs.size(); ++q) {
    const long long* off = hoff[q].data();
    long long p = 0, forced = 0;             // forced > 0: candidate limit of a tile that is being run again after an overflow
    bool compacted_for_tile = false;
    while (p < np) {
      if (off[np] == off[p]) break;          // nothing left in this segment
      if (off[p + 1] - off[p] > capacity - count) { if ((rc = compact())) return rc; }      // count > K + SHOR_SEL_CAP here, so this frees the room
      const long long free_ = capacity - count, base = std::min(free_, probe);
      long long L = forced > 0 ? forced : (long long)std::min((double)TILE_MAX, std::max((double)base, (double)base * gain));
      long long p1 = (long long)(std::upper_bound(off + p + 1, off + np + 1, off[p] + L) - off) - 1;      // last p1 with off[p1] - off[p] <= L
      if (p1 <= p) p1 = p + 1;
      const long long c = off[p1] - off[p];
      if (c == 0) { p = p1; continue; }
      omc_shor_launch_enum_stream(n, m, h->shor_W, h->sbits.as<uint64_t>(), segs[q].kind, segs[q].la, segs[q].lb, p, p1, h->bXin.as<double>(), k,
                                  h->sexist.as<uint64_t>(), n_existing_keys, thi, tlo, h->shi.as<uint64_t>(), h->slo.as<uint64_t>(), d_count,
                                  (unsigned long long)capacity, d_flag, h->stream);
      HIPCHK(hipGetLastError());
      unsigned long long w[2] = {0, 0};
      HIPCHK(hipMemcpyAsync(w, d_count, 16, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
      if ((unsigned int)w[1] != 0 || (long long)w[0] > capacity) {
        // overflow: the tile is discarded.  Once, the buffer is compacted (if it holds anything new) and the same tile run again under the
        // raised threshold; after that the tile is halved until it fits -- one pair always does
        if ((rc = set_count(count))) return rc;
        if (!compacted_for_tile && count > K && count != compacted_at) { if ((rc = compact())) return rc; compacted_for_tile = true; forced = c; }
        else forced = std::max(c / 2, 1LL);
        continue;
      }
      const long long s = (long long)w[0] - count;
      count = (long long)w[0];
      ++h->shor_sel[1];
      gain = (double)c / (2.0 * (double)std::max(s, 1LL));
      p = p1; forced = 0; compacted_for_tile = false;
      if (count > K && count > compacted_at && (count - compacted_at > std::min(capacity, probe) / 2 || count > capacity / 2)) { if ((rc = compact())) return rc; }
      if (2 * s > c) probe = std::min(2 * probe, nominal);
    }
  }
  if (count < K) return fail(OMC_ERR_ARGUMENT, "internal: streaming selection kept fewer keys than requested");
  uint64_t bhi, blo;
  return shor_select_emit(h, count, K, &bhi, &blo, got);
}

int omc_violated_shor_minors(omc_instance* h, const double* X, int n_classes, const int* num_entries_present, int64_t n_existing,
                             const int64_t* existing, int n_minors, double* scores, int64_t* minors, int* n_out) {
  if (!h || !X || (n_classes > 0 && !num_entries_present) || (n_existing > 0 && !existing) || !n_out) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  if (n_minors < 0 || n_existing < 0) return fail(OMC_ERR_ARGUMENT, "negative count");
  if (n_minors > 0 && (!scores || !minors)) return fail(OMC_ERR_ARGUMENT, "NULL output");
  *n_out = 0;
  int rc = shor_prepare(h);
  if (rc) return rc;
  const int n = h->n, m = h->m, k = h->k;
  std::vector<ShorSeg> segs;
  shor_segments(n_classes, num_entries_present, true, segs);   // setdiff! also removes duplicates (OMC.jl:2626)
  std::vector<long long> tot(segs.size(), 0);
  long long N = 0;
  for (size_t q = 0; q < segs.size(); ++q) { if ((rc = shor_scan(h, segs[q], 0, &tot[q]))) return rc; N += tot[q]; }
  const long long budget = (long long)std::max(h->tun.shor_select_kb, 0) * 1024;
  const bool stream = budget > 0 && N > budget / 16;           // 16 bytes of key per candidate
  h->shor_sel[0] = stream ? 1 : 0; h->shor_sel[1] = h->shor_sel[2] = h->shor_sel[3] = 0;
  if (N == 0 || n_minors == 0) return 0;
  // keys of the existing constraints, sorted and unique
  std::vector<uint64_t> ex; ex.reserve((size_t)n_existing);
  for (int64_t e = 0; e < n_existing; ++e) {
    const int64_t i1 = existing[4 * e] - 1, i2 = existing[4 * e + 1] - 1, j1 = existing[4 * e + 2] - 1, j2 = existing[4 * e + 3] - 1;
    if (i1 < 0 || i1 >= n || i2 < 0 || i2 >= n || j1 < 0 || j1 >= m || j2 < 0 || j2 >= m) continue;   // cannot equal any candidate
    ex.push_back((((uint64_t)i1 * n + i2) * m + j1) * m + j2 + 1);
  }
  std::sort(ex.begin(), ex.end()); ex.erase(std::unique(ex.begin(), ex.end()), ex.end());
  if ((rc = upload(h->sexist, ex.data(), ex.size() * 8, h->stream))) return rc;
  if ((rc = upload(h->bXin, X, sizeof(double) * (size_t)k * n * m, h->stream))) return rc;
  EventPair ev;
  if (ev.create()) return fail(999, "hipEventCreate failed");
  hipEvent_t e0 = ev.e0, e1 = ev.e1;
  long long K = 0; unsigned long long got = 0;
  if (stream) {
    // the excluded candidates are the distinct existing tuples that are candidates of a requested class: counted here, not per candidate
    bool want[5] = {false, false, false, false, false};
    for (int c = 0; c < n_classes; ++c) if (num_entries_present[c] >= 0 && num_entries_present[c] <= 4) want[num_entries_present[c]] = true;
    long long excluded = 0;
    for (uint64_t key : ex) {
      uint64_t r = key - 1;
      const uint64_t j2 = r % m; r /= m;
      const uint64_t j1 = r % m; r /= m;
      const uint64_t i2 = r % n, i1 = r / n;
      if (!(i1 < i2 && j1 < j2)) continue;
      const int pc = h->mask[(size_t)j1 * n + i1] + h->mask[(size_t)j2 * n + i1] + h->mask[(size_t)j1 * n + i2] + h->mask[(size_t)j2 * n + i2];
      if (want[pc]) ++excluded;
    }
    K = std::min<long long>(n_minors, N - excluded);            // fewer candidates than n_minors: all of them, sorted (OMC.jl:2634-2635)
    HIPCHK(hipEventRecord(e0, h->stream));
    if (K > 0 && (rc = shor_stream_select(h, segs, (long long)ex.size(), K, budget, &got))) return rc;
  } else {
    if ((rc = h->shi.ensure((size_t)N * 8)) || (rc = h->slo.ensure((size_t)N * 8))) return rc;
    h->shor_sel[3] = 16 * N;
    HIPCHK(hipMemsetAsync(h->scnt.p, 0, 16, h->stream));
    HIPCHK(hipEventRecord(e0, h->stream));
    long long base = 0;
    for (size_t q = 0; q < segs.size(); ++q) {
      long long t = 0;
      if ((rc = shor_scan(h, segs[q], base, &t))) return rc;
      omc_shor_launch_enum_keys(n, m, h->shor_W, h->sbits.as<uint64_t>(), segs[q].kind, segs[q].la, segs[q].lb, h->soff.as<long long>(),
                                h->shor_pairs, h->bXin.as<double>(), k, h->sexist.as<uint64_t>(), (long long)ex.size(),
                                h->shi.as<uint64_t>(), h->slo.as<uint64_t>(), h->scnt.as<unsigned long long>(), h->stream);
      HIPCHK(hipGetLastError());
      base += t;
    }
    unsigned long long excluded = 0;
    HIPCHK(hipMemcpyAsync(&excluded, h->scnt.p, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    K = std::min<long long>(n_minors, N - (long long)excluded);  // fewer candidates than n_minors: all of them, sorted (OMC.jl:2634-2635)
    uint64_t bhi, blo;
    if (K > 0 && (rc = shor_select_emit(h, N, K, &bhi, &blo, &got))) return rc;
  }
  if (K > 0) {
    HIPCHK(hipEventRecord(e1, h->stream));
    std::vector<uint64_t> ohi(got), olo(got);
    HIPCHK(hipMemcpyAsync(ohi.data(), h->sohi.p, got * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(olo.data(), h->solo.p, got * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<size_t> ord(got);
    for (size_t i = 0; i < got; ++i) ord[i] = i;
    std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return ohi[a] != ohi[b] ? ohi[a] > ohi[b] : olo[a] > olo[b]; });
    for (long long r = 0; r < K; ++r) {
      const size_t i = ord[(size_t)r];
      double sc; memcpy(&sc, &ohi[i], 8);
      scores[r] = sc;
      uint64_t key = olo[i] - 1;
      const uint64_t j2 = key % m; key /= m;
      const uint64_t j1 = key % m; key /= m;
      const uint64_t i2 = key % n; const uint64_t i1 = key / n;
      minors[4 * r] = (int64_t)i1 + 1; minors[4 * r + 1] = (int64_t)i2 + 1; minors[4 * r + 2] = (int64_t)j1 + 1; minors[4 * r + 3] = (int64_t)j2 + 1;
    }
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    h->shor_last_ms = ms; h->shor_last_candidates = N;
  }
  *n_out = (int)K;
  return 0;
}

int omc_shor_last_stats(omc_instance* h, double* ms, int64_t* candidates) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (ms) *ms = h->shor_last_ms;
  if (candidates) *candidates = h->shor_last_candidates;
  return 0;
}

int omc_shor_last_select_stats(omc_instance* h, int64_t out[4]) {
  if (!h || !out) return fail(OMC_ERR_ARGUMENT, "handle or out is NULL");
  for (int i = 0; i < 4; ++i) out[i] = h->shor_sel[i];
  return 0;
}

