// Host check of csrc/omc_walks.h: every walk that sizes and places a packed device buffer of the host API, run as the library runs it -- once
// over a measuring Carve, then over a real allocation of exactly the measured size (aligned to 256 bytes as a device allocation is).  Every
// array of the placed walk -- from the pointer the walk handed out to the next one, or to the end of the walk -- is written end to end, so
// the address sanitiser sees any array that leaves the allocation.  For each line of dimensions on stdin the program prints, per walk, the
// two totals and, in walk order, the offset of every pointer the walk filled with the alignment of its type; tests/test_carve_cpu.py does
// the asserting.  Nothing of HIP is linked: the headers are read for their types only.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <type_traits>
#include <string>
#include <vector>

#include "omc_walks.h"

namespace {
char* g_base = nullptr;
struct Field { const char* name; const void* p; size_t align; };
#define F(x) Field{#x, (const void*)(x), alignof(std::remove_pointer_t<decltype(x)>)}

// measure, allocate exactly, place, write every array, print
void run(const char* name, const std::function<void(Carve&)>& walk, const std::function<std::vector<Field>()>& fields) {
  Carve measure;
  walk(measure);
  const size_t bytes = measure.bytes();
  void* mem = nullptr;
  if (posix_memalign(&mem, 256, bytes ? bytes : 1)) { fprintf(stderr, "allocation of %zu bytes failed\n", bytes); exit(2); }
  g_base = (char*)mem;
  Carve place(mem);
  walk(place);
  printf("walk %s %zu %zu\n", name, bytes, place.bytes());
  const std::vector<Field> fl = fields();
  std::vector<size_t> starts;
  for (const Field& f : fl) {
    printf("field %s %td %zu\n", f.name, f.p ? (const char*)f.p - g_base : (ptrdiff_t)-1, f.align);
    if (f.p) starts.push_back((size_t)((const char*)f.p - g_base));
  }
  starts.push_back(place.bytes());
  std::sort(starts.begin(), starts.end());
  for (size_t i = 0; i + 1 < starts.size(); ++i) memset(g_base + starts[i], 0x5a, starts[i + 1] - starts[i]);      // out of bounds if the passes disagree
  free(mem);
}

void stage(const StageDims& d, bool shor, bool keep, bool accel) {
  OmcWS w;
  memset(&w, 0, sizeof(w));
  run("gap", [&](Carve& c) { walk_gap(c, d, w); }, [&] { return std::vector<Field>{F(w.gap_prev), F(w.gap_rate)}; });
  run("small_cone", [&](Carve& c) { walk_small_cone(c, d, w); },
      [&] { return std::vector<Field>{F(w.Vt), F(w.D3V), F(w.W3V), F(w.Q3V), F(w.D3T), F(w.W3T), F(w.Q3T)}; });
  run("objcol", [&](Carve& c) { walk_objcol(c, d, w); }, [&] { return std::vector<Field>{F(w.objcol), F(w.c0col)}; });
  run("check", [&](Carve& c) { walk_check(c, d, w); }, [&] { return std::vector<Field>{F(w.chk_scratch), F(w.stamps)}; });
  run("scalars", [&](Carve& c) { walk_scalars(c, d, w); }, [&] {
    return std::vector<Field>{F(w.obj), F(w.objout), F(w.lb), F(w.c0), F(w.evsum), F(w.cpen), F(w.cst), F(w.rp), F(w.rd), F(w.lmin), F(w.objprev), F(w.lbprev), F(w.fro2), F(w.bfac)};
  });
  run("slot_ints", [&](Carve& c) { walk_slot_ints(c, d, w); }, [&] {
    return std::vector<Field>{F(w.rowov), F(w.status), F(w.iters), F(w.sweeps), F(w.stall), F(w.vvalid), F(w.nbump), F(w.lastbump), F(w.done), F(w.ws_need)};
  });
  run("slot_map", [&](Carve& c) { walk_slot_map(c, d, w.node_of, w.init, w.fin); }, [&] { return std::vector<Field>{F(w.node_of), F(w.init), F(w.fin)}; });
  run("sub_doubles", [&](Carve& c) { walk_sub_doubles(c, d, w); }, [&] { return std::vector<Field>{F(w.sub_theta), F(w.trM), F(w.V3)}; });
  run("sub_ints", [&](Carve& c) { walk_sub_ints(c, d, w); }, [&] {
    return std::vector<Field>{F(w.sub_on), F(w.cone_done), F(w.sub_stat), F(w.sub_wait), F(w.sub_nfail), F(w.v3valid), F(w.ws_first), F(w.w1_fac)};
  });
  run("subC_doubles", [&](Carve& c) { walk_subC_doubles(c, d, w); }, [&] { return std::vector<Field>{F(w.sub_thetaC), F(w.trMc), F(w.lb_est)}; });
  run("subC_ints", [&](Carve& c) { walk_subC_ints(c, d, w); }, [&] { return std::vector<Field>{F(w.sub_onC), F(w.confirm), F(w.sep_done)}; });
  if (accel)
    run("aa_ints", [&](Carve& c) { walk_aa_ints(c, d, w); },
        [&] { return std::vector<Field>{F(w.aa_hist), F(w.aa_head), F(w.aa_pending), F(w.aa_valid), F(w.aa_nacc), F(w.aa_nrej)}; });
  run("out_scalars", [&](Carve& c) { walk_out_scalars(c, d, w); }, [&] { return std::vector<Field>{F(w.oobj), F(w.olb), F(w.olmin), F(w.orho)}; });
  run("out_ints", [&](Carve& c) { walk_out_ints(c, d, w); }, [&] { return std::vector<Field>{F(w.ostatus), F(w.oiters)}; });
  if (keep) {
    const size_t cnnz = shor ? 0 : d.nnz;
    run("cert_slot", [&](Carve& c) { walk_cert_slot(c, d, cnnz, w); },
        [&] { return std::vector<Field>{F(w.cb_rho), F(w.cbBound), F(w.cbLam), F(w.cblam), F(w.cbPsi)}; });
    run("cert_flags", [&](Carve& c) { walk_cert_flags(c, d, w); }, [&] { return std::vector<Field>{F(w.cert_flag), F(w.cert_have)}; });
    run("cert_node", [&](Carve& c) { walk_cert_node(c, d, cnnz, w); }, [&] { return std::vector<Field>{F(w.ocBound), F(w.ocLam), F(w.oclam), F(w.ocPsi)}; });
  }
}

void shor_stage(size_t S, size_t N, size_t nq1, size_t m, size_t nm) {
  ShWS sh;
  OmcWS wb;
  memset(&sh, 0, sizeof(sh));
  memset(&wb, 0, sizeof(wb));
  run("shor_fro", [&](Carve& c) { walk_shor_fro(c, S, sh); }, [&] { return std::vector<Field>{F(sh.fro2B), F(sh.trB)}; });
  run("shor_cert_slot", [&](Carve& c) { walk_shor_cert(c, S, nq1, m, nm, sh.cbGam, sh.cbZeta, sh.cbXi, sh.cbXbar); },
      [&] { return std::vector<Field>{F(sh.cbGam), F(sh.cbZeta), F(sh.cbXi), F(sh.cbXbar)}; });
  run("shor_cert_node", [&](Carve& c) { walk_shor_cert(c, N, nq1, m, nm, sh.ocGam, sh.ocZeta, sh.ocXi, sh.ocXbar); },
      [&] { return std::vector<Field>{F(sh.ocGam), F(sh.ocZeta), F(sh.ocXi), F(sh.ocXbar)}; });
  run("shor_sub_ints", [&](Carve& c) { walk_shor_sub_ints(c, S, sh, wb); },
      [&] { return std::vector<Field>{F(sh.sub_onB), F(sh.cone_doneB), F(sh.sub_waitB), F(sh.sub_nfailB), F(wb.sub_stat)}; });
}

// in walk order; Lam exists in the base evaluator only
std::vector<Field> eval_double_fields(const OmcWS& w, const EvalArrays& a) {
  std::vector<Field> f = {F(w.rcoef), F(w.rrhs), F(w.cutx), F(w.Qb)};
  if (a.Lam) f.push_back(F(a.Lam));
  for (const Field& e : {F(a.lam), F(a.Psi), F(a.T1), F(w.chk_scratch), F(w.c0), F(w.cpen), F(w.cst), F(w.fro2c), F(w.evsum), F(a.scalars_end)}) f.push_back(e);
  return f;
}
std::vector<Field> eval_int_fields(const OmcWS& w, const EvalArrays& a) {
  return {F(w.R), F(w.rr), F(w.rkind), F(w.rcut), F(w.rbi), F(w.rbj), F(w.done), F(w.vvalidC), F(w.sweeps), F(w.mw_stat), F(a.zero_end)};
}

void dual(const EvalDims& d) {
  OmcWS w;
  memset(&w, 0, sizeof(w));
  EvalArrays a{};
  run("dual_matrices", [&](Carve& c) { walk_dual_matrices(c, d, w); }, [&] { return std::vector<Field>{F(w.MbufC), F(w.VrowC), F(w.Mchk)}; });
  run("dual_doubles", [&](Carve& c) { walk_dual_doubles(c, d, w, a); }, [&] { return eval_double_fields(w, a); });
  run("dual_ints", [&](Carve& c) { walk_dual_ints(c, d, w, a); }, [&] { return eval_int_fields(w, a); });
}

void scert(const ScertDims& s, const EvalDims& d) {
  OmcWS w;
  ShorCertWS sc;
  memset(&w, 0, sizeof(w));
  memset(&sc, 0, sizeof(sc));
  ScertArrays in{};
  EvalArrays a{};
  run("scert_doubles", [&](Carve& c) { walk_scert_doubles(c, s, d, sc, in, w, a); }, [&] {
    std::vector<Field> f = {F(in.scale), F(in.Gam), F(in.zeta), F(in.xi), F(in.Xbar)};      // in walk order
    if (s.store_clean) f.push_back(F(sc.GamC));
    for (const Field& e : {F(sc.cleanpart), F(sc.e1), F(sc.e2), F(sc.row8), F(sc.minpart), F(sc.lamDX), F(sc.c0col), F(sc.colmu), F(w.MbufC), F(w.VrowC), F(w.Mchk)})
      f.push_back(e);
    if (s.slab) f.push_back(F(w.cone_scratch));
    for (const Field& e : eval_double_fields(w, a)) f.push_back(e);
    return f;
  });
  run("scert_ints", [&](Carve& c) { walk_scert_ints(c, s, d, sc, in, w, a); }, [&] {
    std::vector<Field> f = {F(in.node_group), F(in.view_node), F(in.view_way), F(sc.colbad)};
    for (const Field& e : eval_int_fields(w, a)) f.push_back(e);
    return f;
  });
}

void project(size_t B, size_t NP) {
  OmcWS w;
  memset(&w, 0, sizeof(w));
  int* ints_end = nullptr;
  run("project_doubles", [&](Carve& c) { walk_project_doubles(c, B, NP, w); }, [&] { return std::vector<Field>{F(w.fro2), F(w.ev_out)}; });
  run("project_ints", [&](Carve& c) { walk_project_ints(c, B, w, ints_end); },
      [&] { return std::vector<Field>{F(w.done), F(w.vvalid), F(w.sweeps), F(w.mw_stat), F(ints_end)}; });
}
}  // namespace

int main() {
  char line[512];
  while (fgets(line, sizeof(line), stdin)) {
    char kind[32];
    unsigned long long v[16] = {0};
    const int got = sscanf(line, "%31s %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu", kind, v, v + 1, v + 2, v + 3, v + 4, v + 5,
                           v + 6, v + 7, v + 8, v + 9, v + 10, v + 11, v + 12, v + 13, v + 14, v + 15);
    if (got < 1) continue;
    const std::string k = kind;
    printf("case %s", line);
    if (k == "stage" && got == 12) stage(StageDims{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]}, v[8] != 0, v[9] != 0, v[10] != 0);
    else if (k == "shor" && got == 6) shor_stage(v[0], v[1], v[2], v[3], v[4]);
    else if (k == "dual" && got == 8) dual(EvalDims{v[0], v[1], v[2], v[3], v[4], v[5], v[6]});
    else if (k == "scert" && got == 15)
      scert(ScertDims{v[0], v[8], v[9], v[10], v[11], v[3], v[12], v[13] != 0}, EvalDims{v[1], v[2], 1, v[4], v[5], v[6], v[7]});
    else if (k == "project" && got == 3) project(v[0], v[1]);
    else { fprintf(stderr, "bad line: %s", line); return 1; }
  }
  return 0;
}
