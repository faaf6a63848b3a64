// omc_api_comm.cpp -- the RCCL communicator behind the C ABI of include/omc.h: omc_comm_unique_id, omc_comm_init, omc_allreduce_bounds,
// omc_bcast_incumbent, omc_allgather_records, omc_comm_destroy.  The only source that sees <rccl/rccl.h> and <dlfcn.h>.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <string>
#include <vector>

#include "omc_api_internal.h"
#include <dlfcn.h>
#include <rccl/rccl.h>   // types only: the library is loaded with dlopen on first use, so that libomc_hip.so has no hard dependency on it

namespace {
struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl g_rccl;
int rccl_load() {
  if (g_rccl.lib) return 0;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void* lib = nullptr;
  for (const char* nm : names) { lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL); if (lib) break; }
  if (!lib) return fail(OMC_ERR_COMM, std::string("librccl not loadable: ") + (dlerror() ? dlerror() : "?"));
  Rccl r; r.lib = lib;
  r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(lib, "ncclGetUniqueId");
  r.CommInitRank = (decltype(r.CommInitRank))dlsym(lib, "ncclCommInitRank");
  r.AllReduce = (decltype(r.AllReduce))dlsym(lib, "ncclAllReduce");
  r.Broadcast = (decltype(r.Broadcast))dlsym(lib, "ncclBroadcast");
  r.AllGather = (decltype(r.AllGather))dlsym(lib, "ncclAllGather");
  r.CommDestroy = (decltype(r.CommDestroy))dlsym(lib, "ncclCommDestroy");
  r.GetErrorString = (decltype(r.GetErrorString))dlsym(lib, "ncclGetErrorString");
  if (!r.GetUniqueId || !r.CommInitRank || !r.AllReduce || !r.Broadcast || !r.AllGather || !r.CommDestroy) return fail(OMC_ERR_COMM, "librccl lacks an expected symbol");
  g_rccl = r;
  return 0;
}
int rccl_fail(ncclResult_t e, const char* what) {
  return fail(OMC_ERR_COMM, std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(e) : "RCCL error"));
}
}  // namespace

int omc_comm_unique_id(void* id_out) {
  if (!id_out) return fail(OMC_ERR_ARGUMENT, "id_out is NULL");
  int rc = rccl_load(); if (rc) return rc;
  ncclUniqueId id;
  ncclResult_t e = g_rccl.GetUniqueId(&id);
  if (e != ncclSuccess) return rccl_fail(e, "ncclGetUniqueId");
  static_assert(sizeof(ncclUniqueId) == OMC_COMM_ID_BYTES, "unique id size");
  memcpy(id_out, &id, sizeof(id));
  return 0;
}

int omc_comm_init(omc_instance* h, int rank, int world_size, const void* id) {
  if (!h || !id) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  if (world_size < 1 || rank < 0 || rank >= world_size) return fail(OMC_ERR_ARGUMENT, "rank / world_size out of range");
  if (h->comm) return fail(OMC_ERR_ARGUMENT, "communicator already initialised");
  int rc = rccl_load(); if (rc) return rc;
  HIPCHK(hipSetDevice(h->device));
  ncclUniqueId uid; memcpy(&uid, id, sizeof(uid));
  ncclComm_t c = nullptr;
  ncclResult_t e = g_rccl.CommInitRank(&c, world_size, uid, rank);
  if (e != ncclSuccess) return rccl_fail(e, "ncclCommInitRank");
  h->comm = (void*)c; h->comm_rank = rank; h->comm_world = world_size;
  if ((rc = h->bcomm.ensure(64))) return rc;
  return 0;
}

int omc_allreduce_bounds(omc_instance* h, double* ub, double* lb, int* owner) {
  if (!h || !ub || !lb) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  if (!h->comm) return fail(OMC_ERR_COMM, "omc_comm_init has not been called on this handle");
  HIPCHK(hipSetDevice(h->device));
  double* d = h->bcomm.as<double>();
  const double mine = *ub;
  double v[2] = {*ub, *lb};
  HIPCHK(hipMemcpyAsync(d, v, 16, hipMemcpyHostToDevice, h->stream));
  ncclResult_t e = g_rccl.AllReduce(d, d, 2, ncclDouble, ncclMin, (ncclComm_t)h->comm, h->stream);
  if (e != ncclSuccess) return rccl_fail(e, "ncclAllReduce(min, fp64[2])");
  HIPCHK(hipMemcpyAsync(v, d, 16, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  *ub = v[0]; *lb = v[1];
  if (owner) {   // second 8-byte MIN: the smallest rank that holds the minimum (ties are common: every rank starts from the same root bound)
    double r = (mine == v[0]) ? (double)h->comm_rank : (double)h->comm_world;
    HIPCHK(hipMemcpyAsync(d + 2, &r, 8, hipMemcpyHostToDevice, h->stream));
    e = g_rccl.AllReduce(d + 2, d + 2, 1, ncclDouble, ncclMin, (ncclComm_t)h->comm, h->stream);
    if (e != ncclSuccess) return rccl_fail(e, "ncclAllReduce(min, owner)");
    HIPCHK(hipMemcpyAsync(&r, d + 2, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *owner = (int)r;
  }
  return 0;
}

int omc_bcast_incumbent(omc_instance* h, int root, double* X) {
  if (!h || !X) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  if (!h->comm) return fail(OMC_ERR_COMM, "omc_comm_init has not been called on this handle");
  if (root < 0 || root >= h->comm_world) return fail(OMC_ERR_ARGUMENT, "root out of range");
  HIPCHK(hipSetDevice(h->device));
  const size_t cnt = (size_t)h->n * h->m;
  int rc = h->bXin.ensure(8 * cnt + 64); if (rc) return rc;
  double* d = h->bXin.as<double>();
  if (h->comm_rank == root) HIPCHK(hipMemcpyAsync(d, X, 8 * cnt, hipMemcpyHostToDevice, h->stream));
  ncclResult_t e = g_rccl.Broadcast(d, d, cnt, ncclDouble, root, (ncclComm_t)h->comm, h->stream);
  if (e != ncclSuccess) return rccl_fail(e, "ncclBroadcast(X)");
  if (h->comm_rank != root) HIPCHK(hipMemcpyAsync(X, d, 8 * cnt, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// The per-node records every rank needs to grow the same tree (the serial loop OMC.jl:700-719 sees every relaxed node: status, objective,
// bound, eigenvalues, breakpoint vector, U -- 8 (6 + n + n k) bytes per node, never X or Y): all-gather of `cnt` rows of `width` doubles per rank.
// Ranks may hold different counts: the counts are gathered first (8 bytes per rank), the rows are padded to the largest count, and
// `out` receives the rows of rank 0, then rank 1, ... (sum of counts x width doubles; capacity = world x max_cnt_capacity rows).
int omc_allgather_records(omc_instance* h, const double* rows, int cnt, int width, double* out, int out_capacity_rows, int* counts /* world */) {
  if (!h || !out || !counts || (cnt > 0 && !rows)) return fail(OMC_ERR_ARGUMENT, "NULL argument");
  if (cnt < 0 || width <= 0) return fail(OMC_ERR_ARGUMENT, "cnt / width out of range");
  if (!h->comm) return fail(OMC_ERR_COMM, "omc_comm_init has not been called on this handle");
  HIPCHK(hipSetDevice(h->device));
  const int W = h->comm_world;
  int rc = h->bcomm.ensure(64 + 8 * (size_t)W); if (rc) return rc;
  double* d = h->bcomm.as<double>();
  const double mine = (double)cnt;
  HIPCHK(hipMemcpyAsync(d + 4, &mine, 8, hipMemcpyHostToDevice, h->stream));
  ncclResult_t e = g_rccl.AllGather(d + 4, d + 8, 1, ncclDouble, (ncclComm_t)h->comm, h->stream);
  if (e != ncclSuccess) return rccl_fail(e, "ncclAllGather(counts)");
  std::vector<double> hc(W);
  HIPCHK(hipMemcpyAsync(hc.data(), d + 8, 8 * (size_t)W, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  int cmax = 0; long tot = 0;
  for (int r = 0; r < W; ++r) { counts[r] = (int)hc[r]; cmax = std::max(cmax, counts[r]); tot += counts[r]; }
  if (tot > out_capacity_rows) return fail(OMC_ERR_ARGUMENT, "omc_allgather_records: out is too small for the gathered rows");
  if (cmax == 0) return 0;
  const size_t blk = (size_t)cmax * width;
  if ((rc = h->bXin.ensure(8 * blk * (size_t)(W + 1) + 64))) return rc;
  double* send = h->bXin.as<double>(); double* recv = send + blk;
  HIPCHK(hipMemsetAsync(send, 0, 8 * blk, h->stream));
  if (cnt) HIPCHK(hipMemcpyAsync(send, rows, 8 * (size_t)cnt * width, hipMemcpyHostToDevice, h->stream));
  e = g_rccl.AllGather(send, recv, blk, ncclDouble, (ncclComm_t)h->comm, h->stream);
  if (e != ncclSuccess) return rccl_fail(e, "ncclAllGather(records)");
  size_t o = 0;
  for (int r = 0; r < W; ++r) {
    if (counts[r]) HIPCHK(hipMemcpyAsync(out + o, recv + (size_t)r * blk, 8 * (size_t)counts[r] * width, hipMemcpyDeviceToHost, h->stream));
    o += (size_t)counts[r] * width;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int omc_comm_destroy(omc_instance* h) {
  if (!h) return fail(OMC_ERR_ARGUMENT, "handle is NULL");
  if (h->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy((ncclComm_t)h->comm);
  h->comm = nullptr; h->comm_rank = 0; h->comm_world = 1;
  return 0;
}
