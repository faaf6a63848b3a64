// omc_branch.h -- descriptors of a finished node's children built on the device (omc_relax_append_children; omc_branch.hip): what the two
// kernels take beside the workspace, and their launcher.  A child is its parent's descriptor plus one cut: x = the parent's breakpoint vector
// (OmcWS::obx), Uhat = its U (OmcWS::oU), so 2k + 1 rows and at most one column of the row basis Q are new.  The results are pack_nodes'
// (omc_api.cpp) bit for bit: every sum runs in the host's index order on one lane, without fused multiply-adds.
#ifndef OMC_BRANCH_H
#define OMC_BRANCH_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "omc_device.h"

#define BRANCH_CHUNK 1024      // children (and so distinct parents) of one pair of launches; a longer call runs in chunks
#define BRANCH_NMAX 4096       // two vectors of n doubles in LDS

struct BranchWS {
  int cut_type, q1;            // of the staged batch (OMC_CUT_*, reference_quirk_q1)
  // scratch, one entry per distinct parent of the chunk (k_branch_basis writes, k_branch_write reads)
  double* vhat;                // k: Uhat' x
  double* q;                   // n: the new column of Q (where keep)
  int* keep;                   // 1: x adds a column to the parent's row basis
  // index image of the chunk, uploaded as one piece laid out by walk_branch_ints
  int* slot_node;              // per parent: its node id
  int* slot_L;                 // per parent: its cuts (the device keeps no count of them)
  int* child_slot;             // per child: its parent's entry in the scratch
  int8_t* dirs;                // per child: k direction codes (OMC_DIR_*)
};

#ifdef __cplusplus
extern "C" {
#endif
// nslots parents, nchildren children written to the nodes first_child ... of the per-node descriptor arrays of w
void omc_launch_branch(const OmcWS* w, const BranchWS* b, int nslots, int first_child, int nchildren, hipStream_t s);
#ifdef __cplusplus
}
#endif
#endif
