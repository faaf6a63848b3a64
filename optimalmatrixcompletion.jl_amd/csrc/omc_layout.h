// omc_layout.h -- working-memory layouts of the large kernels, defined ONCE for both sides: the kernel takes its pointers from the layout
// (offsets in doubles from the start of its block: dynamic LDS or a per-slot global slab), the host takes the block's size from the same
// struct.  omc_plan_geometry turns them into the launch decisions of a workspace (OmcGeom, carried in OmcWS::geo to the launchers).
// The "margins" named below are bytes no kernel addresses: they keep the LDS-or-slab thresholds and slab strides where they were measured.
#ifndef OMC_LAYOUT_H
#define OMC_LAYOUT_H
#include <hip/hip_runtime.h>
#include <stddef.h>

#define NNQP_PMAX 64                                        // passive rows of the row projection (wave_nnqp)
#define NNQP_GP_DOUBLES (NNQP_PMAX * (NNQP_PMAX + 1) / 2)   // its packed Gram matrix: __shared__ s_Gp of k_global and the altmin kernels
#define NNQP_STATIC_BYTES ((NNQP_GP_DOUBLES + 2 * NNQP_PMAX) * 8 + NNQP_PMAX * 4)      // s_Gp, s_sv, s_tmp, s_pl
#define OMC_MAX_DYN_LDS (144 * 1024)
#define SUBP 16    // tracked subspace dimension of k_cone_sub
#define GL_XS 16   // cut vectors staged per pass of k_global (one MFMA column block)
#define OMC_HD __host__ __device__ inline
// ---- eigen-kernels: G (Np columns, leading dimension ld), squared norms (Np), weights (Np), selection (ints) ---------------------------
struct ConeLayout { int Np, ld; size_t ev, wgt, sel; };
OMC_HD ConeLayout cone_carve(int N, int ld) { const int Np = (N + 1) & ~1; const size_t ev = (size_t)Np * ld; return {Np, ld, ev, ev + Np, ev + 2 * Np}; }
// k_cone (cold Jacobi): ld = Np | 1, Np ints, 16 bytes of margin
OMC_HD ConeLayout cone_layout(int N) { return cone_carve(N, ((N + 1) & ~1) | 1); }
OMC_HD size_t cone_bytes(int N) { const ConeLayout L = cone_layout(N); return L.sel * 8 + (size_t)L.Np * 4 + 16; }
// k_cone_ws (warm-started Jacobi): ld from ws_geometry, Np + 2 ints; margin: Np doubles and 64 bytes
OMC_HD size_t ws_bytes(int N, int ld) { const ConeLayout L = cone_carve(N, ld); return (L.sel + L.Np) * 8 + (size_t)(L.Np + 2) * 4 + 64; }
OMC_HD int ws_rpl(int N, int lpp) { return (((N + lpp - 1) / lpp) + 1) & ~1; }      // rows per lane: even, a lane owns contiguous rows
// Geometry at order N: lanes per pair so that 512 threads cover the N/2 pairs, rows padded to lpp*rpl (<= 20 rows per lane).  G lives in LDS
// when it fits, else in a per-slot global slab (L2 resident) with 16 lanes per pair (a wave per pair at orders 513 .. 1024).
// lpp = 0: more than 32 rows per lane, beyond the kernel (WS_JROWS).
struct WsGeometry { int lpp, rpl, ld, use_lds; size_t bytes; };      // bytes: of the LDS block or of the slab
OMC_HD WsGeometry ws_geometry(int N) {
  const int Np2 = (N + 1) & ~1;
  int lpp = 16; while (lpp > 4 && lpp * (Np2 / 2) > 512) lpp >>= 1;
  int rpl = ws_rpl(N, lpp), Nrp = rpl * lpp;
  int ld = Nrp + ((16 - (Nrp & 31)) & 31);                        // 16 (mod 32): neighbouring columns start 32 LDS banks apart
  if (ws_bytes(N, ld) > OMC_MAX_DYN_LDS) ld = Nrp + 2;            // does not fit: plain padding
  const int use_lds = ws_bytes(N, ld) <= OMC_MAX_DYN_LDS;
  if (!use_lds) {
    lpp = 16; rpl = ws_rpl(N, 16);
    if (rpl > 32 && N <= 1024) { lpp = 64; rpl = ws_rpl(N, 64); }
    ld = rpl * lpp + 2;
  }
  return {rpl <= 32 ? lpp : 0, rpl, ld, use_lds, ws_bytes(N, ld)};
}
// ---- k_setup_gram: the R (R + 1) / 2 pairs (r, s), r <= s, of a node's R rows numbered row by row -- (0,0), (0,1), .., (0,R-1), (1,1), .. --
// and cut into chunks of GRAM_CHUNK consecutive pairs, one workgroup each ------------------------------------------------------------------
#define GRAM_CHUNK 8
#define CB_XS 4096   // doubles of cut vectors that k_check_build stages in LDS (the host clamps OMC_CHECK_XS to it)
OMC_HD int gram_npairs(int R) { return R * (R + 1) / 2; }
OMC_HD int gram_chunks(int R) { return (gram_npairs(R) + GRAM_CHUNK - 1) / GRAM_CHUNK; }
OMC_HD void gram_pair_of(int p, int R, int* r, int* s) {      // p < gram_npairs(R)
  int rr = 0;
  while (p >= R - rr) { p -= R - rr; ++rr; }
  *r = rr; *s = rr + p;
}
OMC_HD void gram_pair_next(int R, int* r, int* s) { if (++*s == R) { ++*r; *s = *r; } }
// ---- multi-workgroup eigen-kernels (omc_cone_mw.hip), per-slot global slab: G (Ncp columns of ld doubles; columns padded to whole block
// pairs, rows to 16), squared norms ev, eigenvalues lam, weights wgt (Ncp each), selection sel (Ncp ints), the largest squared relative
// cross product of each sweep smax (MW_MAXSW 64-bit words), head (base, then nsel and nkeep as ints).  The plain sequence (CONE_SEP, CONE_TOPK:
// omc_launch_cone_plain_mw) selects no weights and keeps the partial sums of squares of its input, one per 16-row tile (NP / 16 <= Ncp),
// in the words of wgt: fro names them ----------------------------------------------------------------------------------------------------------
#define MW_B 16         // columns per block: one v_mfma_f64_16x16x4_f64 tile, a 32 x 32 Gram matrix per pair
#define MW_MAXSW 32     // sweep slots of smax: the sweep budget of a call never exceeds it
#define MW_MIN_ORDER 145   // below, k_cone_ws holds G in LDS: the multi-workgroup path is never planned there
#define MW_MAX_ORDER 4096
#define MW_TAU_PLAIN 1e-14   // rotation threshold and stop rule of the plain sequence: the cold kernel's (eig_frontend), omc_plain_multi_tau()
#define MW_PLAIN_SWEEPS 30   // sweeps it enqueues: MAX_SWEEPS, the cold kernel's limit
struct MwLayout { int ld, Ncp, nb; size_t ev, lam, wgt, sel, smax, head, bytes, fro; };
OMC_HD MwLayout mw_layout(int N) {
  const int NP = (N + 15) & ~15, Ncp = (N + 2 * MW_B - 1) & ~(2 * MW_B - 1), ld = NP + 4;
  static_assert(2 * MW_B >= 16, "fro: the NP / 16 partial sums of the plain sequence lie in the Ncp words of wgt, NP <= Ncp");
  const size_t ev = (size_t)Ncp * ld, sel = ev + 3 * (size_t)Ncp, smax = sel + Ncp / 2, head = smax + MW_MAXSW;
  return {ld, Ncp, Ncp / MW_B, ev, ev + Ncp, ev + 2 * (size_t)Ncp, sel, smax, head, (head + 4) * 8, ev + 2 * (size_t)Ncp};
}
OMC_HD int mw_plain_launches(const MwLayout& L, int sweeps) { return sweeps * (L.nb - 1) + 4; }      // fro, prepare, the rounds, norms, pick
// ---- k_cone_sub: X, then Z (SUBP x LD each; Z in a global slab beyond order 512), 4 partial 16 x 16 products (Cs), Gram / Cholesky /
// Ritz rotation (Hs, 16 x 17), Jacobi work (Gj, 16 x 17), Ritz values (th), squared norms (evj), red (32), wgt (16), sel (16 ints) ------
struct SubLayout { int LD, zglob; size_t Za, Cs, Hs, Gj, th, evj, red, wgt, sel, bytes; };
OMC_HD SubLayout sub_layout(int np16) {
  const int LD = np16 + 2, zglob = np16 > 512; const size_t blk = (size_t)SUBP * LD, Cs = (zglob ? 1 : 2) * blk, th = Cs + 4 * 256 + 2 * 16 * 17;
  return {LD, zglob, blk, Cs, Cs + 4 * 256, Cs + 4 * 256 + 16 * 17, th, th + 16, th + 32, th + 64, th + 80, (th + 80 + 8) * 8};
}
// ---- k_small: T1 = (Y - D3) Q (n x rmax), M3 (ld3 x ld3), Jacobi work Gm (Npm x ldm), ev, wgt (Npm each), sel (Npm ints), recovery
// coefficients Cc (rmax x k, + 2), staged Q' Qs (n x 16, LDS variant only), SMALL_CS doubles for small_proj_chain (the symmetrised M3 and
// the previous eigenvectors, 16 x 16 each, until the sweep starts; then the 16 x 16 copy of dS); 104 bytes of margin ---------------------
#define SMALL_STATIC_LDS 1024      // allowance for the kernel's __shared__ scalars and reduction arrays (528 bytes as compiled)
#define SMALL_CS 512
struct SmallLayout { int ld3; size_t M3, Gm, ev, wgt, sel, Cc, Qs, Cs, bytes; };
OMC_HD SmallLayout small_layout(int n, int rmax, int k) {
  const int ld3 = rmax + k, Npm = (ld3 + 1) & ~1, ldm = Npm | 1;
  const size_t M3 = (size_t)n * rmax, Gm = M3 + (size_t)ld3 * ld3, ev = Gm + (size_t)Npm * ldm, sel = ev + 2 * Npm, Cc = sel + Npm / 2, Qs = Cc + (size_t)rmax * k + 2;
  const size_t Cs = Qs + (size_t)n * 16;
  return {ld3, M3, Gm, ev, ev + Npm, sel, Cc, Qs, Cs, (Cs + SMALL_CS) * 8 + 104};
}
// ---- k_global: packed lower triangle of the target (tY), tU (n x k), tV (rmax x k), cvec, mu (Rmax each), staged cut vectors xs
// (GL_XS x n), qrow (Rmax); 80 bytes of margin --------------------------------------------------------------------------------------------
// static LDS of the kernel: the NNQP scratch plus 2.5 KB for its reduction, selection and staging arrays (2328 bytes as compiled)
#define GLOB_STATIC_LDS ((size_t)NNQP_STATIC_BYTES + 2560)
struct GlobLayout { size_t tU, tV, cvec, mu, xs, qrow, bytes; };
OMC_HD GlobLayout glob_layout(int n, int k, int rmax, int Rmax) {
  const size_t tU = (size_t)n * (n + 1) / 2, tV = tU + (size_t)n * k, cvec = tV + (size_t)rmax * k, xs = cvec + 2 * Rmax, qrow = xs + (size_t)GL_XS * n;
  return {tU, tV, cvec, cvec + Rmax, xs, qrow, (qrow + Rmax) * 8 + 80};
}
// factored W1: k_global stages the accepted Ritz vectors of a slot (at most SUBP, n doubles each) in s_Gp, idle outside its row projection
OMC_HD bool glob_w1_fits(int n) { return (size_t)SUBP * n <= (size_t)NNQP_GP_DOUBLES; }
// ---- k_colprox, per wave.  colprox_reg (LDS, c <= 64 rows): B (packed, kept beside L only with keepB), L, vo, pinv (c each), sidx (c ints in
// 2 c doubles).  colprox_body (global slab, larger columns): B, L, va, vy, vz, vo.  8 doubles of margin each -----------------------------------
struct CpRegLayout { int Lm, vo, pinv, sidx, doubles; };
OMC_HD CpRegLayout cp_reg_layout(int c, int keepB) { const int tri = (c * (c + 1)) >> 1, vo = (keepB ? 2 : 1) * tri; return {keepB ? tri : 0, vo, vo + c, vo + 2 * c, vo + 4 * c + 8}; }
struct CpBodyLayout { size_t Lm, va, vy, vz, vo, doubles; };
OMC_HD CpBodyLayout cp_body_layout(int c) { const size_t tri = (size_t)c * (c + 1) / 2, va = 2 * tri; return {tri, va, va + c, va + 2 * c, va + 3 * c, va + 4 * c + 8}; }
// ---- k_colprox_block (omc_colprox_block.hip), one workgroup per column of c observed rows.  The matrix is a blocked lower triangle of
// nb (nb + 1) / 2 tiles of 16 x 16 doubles, nb = ceil(c / 16); tile (I, J), J <= I, is number I (I + 1) / 2 + J and holds its entry (r, q) at
// q * 16 + r.  LDS variant: the tiles, then the vectors (a, y, z, w, previous alpha: 16 nb doubles each; row indices: 16 nb ints).  Slab
// variant: the tiles live in a per-(slot, column) global slab (slab doubles), the LDS block holds the current panel (nb - 1 tiles) and the
// vectors.  The kernel's static LDS (inverse of the diagonal tile, its factor, reduction words) is CPB_STATIC_LDS bytes at most.
#define CPB_TILE 256
#define CPB_STATIC_LDS 4352
struct CpBlockLayout { int nb, ntiles; size_t panel, va, vy, vz, vw, vo, sidx, doubles, slab; };
OMC_HD int cpb_tile(int I, int J) { return ((I * (I + 1)) >> 1) + J; }
OMC_HD CpBlockLayout cp_block_layout(int c, int lds) {
  const int nb = c > 0 ? (c + 15) >> 4 : 1, nt = (nb * (nb + 1)) >> 1;
  const size_t cp = (size_t)16 * nb, va = (size_t)CPB_TILE * (lds ? nt : (nb > 1 ? nb - 1 : 1));
  return {nb, nt, 0, va, va + cp, va + 2 * cp, va + 3 * cp, va + 4 * cp, va + 5 * cp, va + 5 * cp + cp / 2, lds ? 0 : (size_t)CPB_TILE * nt};
}
OMC_HD int cp_block_fits(int c, int lds) { return cp_block_layout(c, lds).doubles * 8 <= (size_t)OMC_MAX_DYN_LDS; }
OMC_HD int cp_block_lds_cmax() { int nb = 1; while (cp_block_fits(16 * (nb + 1), 1)) ++nb; return 16 * nb; }      // longest column whose tiles fit the LDS (176)
OMC_HD int cp_block_cmax() { int nb = 1; while (cp_block_fits(16 * (nb + 1), 0)) ++nb; return 16 * nb; }          // longest column the slab variant takes (its panel and vectors fit)
// plan for the columns of at least block_min rows among columns of at most cmax: out = {longest LDS column, dynamic LDS bytes of the launch
// that holds a column of cmax rows, slab stride in doubles (0: LDS), workgroups per CU by LDS (160 KiB per CU), 1 if a column of cmax rows
// goes to the block kernel}
OMC_HD void cp_block_plan(int cmax, int block_min, long long* out) {
  const int ldsc = cp_block_lds_cmax(), on = cmax >= block_min && cmax >= 1 && cmax <= cp_block_cmax();
  const CpBlockLayout L = cp_block_layout(cmax, cmax <= ldsc);
  out[0] = ldsc; out[1] = on ? (long long)(L.doubles * 8) : 0; out[2] = on ? (long long)L.slab : 0;
  out[3] = on ? (long long)((160 * 1024) / (L.doubles * 8 + CPB_STATIC_LDS)) : 0; out[4] = on;
}
// ---- altmin kernels (omc_altmin.hip); 8 doubles of margin ---------------------------------------------------------------------------------
struct Altmin1Layout { size_t v, h, g, u0, cvec, mu, bytes; };       // k_altmin (rank 1): u (n), v (m), h, g, u0 (n each), cvec, mu (Rmax each)
OMC_HD Altmin1Layout altmin1_layout(int n, int m, int Rmax) { const size_t h = (size_t)n + m, cvec = h + 3 * n; return {(size_t)n, h, h + n, h + 2 * n, cvec, cvec + Rmax, (cvec + 2 * Rmax + 8) * 8}; }
struct AltminKLayout { size_t ut, u0, g, H, Hinv, v, cvec, mu, bytes; };      // k_altmin_k: u, ut, u0, g (n k each), H, Hinv (n k k each), v (k m), cvec, mu
OMC_HD AltminKLayout altmink_layout(int n, int m, int k, int Rmax) {
  const size_t nk = (size_t)n * k, H = 4 * nk, v = H + 2 * nk * k, cvec = v + (size_t)k * m;
  return {nk, 2 * nk, 3 * nk, H, H + nk * k, v, cvec, cvec + Rmax, (cvec + 2 * Rmax + 8) * 8};
}
// k_altmin_w (ranks 5 .. 8): the state of k_altmin_k, then the multiplier vectors of the dual Newton method (th, th2, q, qt, step, tmp: mq = k^2
// doubles each; act: mq ints), its Jacobian J and model matrix P (mq x mq, leading dimension mq) and the packed Cholesky factor Lc (mq (mq + 1) / 2)
struct AltminWLayout { size_t ut, u0, g, H, Hinv, v, cvec, mu, th, th2, q, qt, step, tmp, act, J, P, Lc, bytes; };
OMC_HD AltminWLayout altminw_layout(int n, int m, int k, int Rmax) {
  const size_t nk = (size_t)n * k, mq = (size_t)k * k, H = 4 * nk, v = H + 2 * nk * k, cvec = v + (size_t)k * m, th = cvec + 2 * Rmax, J = th + 7 * mq, Lc = J + 2 * mq * mq;
  return {nk, 2 * nk, 3 * nk, H, H + nk * k, v, cvec, cvec + Rmax, th, th + mq, th + 2 * mq, th + 3 * mq, th + 4 * mq, th + 5 * mq, th + 6 * mq, J, J + mq * mq, Lc,
          (Lc + mq * (mq + 1) / 2 + 8) * 8};
}
// ---- launch decisions ---------------------------------------------------------------------------------------------------------------------
struct KernelPlan { int use_lds; size_t lds_bytes, slab_stride; };      // launch bytes (0 with the slab) ; slab stride in doubles (0 with LDS)
OMC_HD KernelPlan plan_block(size_t bytes, bool fits) { return {fits ? 1 : 0, fits ? bytes : 0, fits ? 0 : bytes / 8 + 8}; }
// altmin: kernel variant by rank (1: k_altmin, 2: k_altmin_k, 3: k_altmin_w); 8 KB of headroom under the kernel's dynamic budget
// (omc_altmin_set_lds; k_altmin_k holds ~25 KB of static LDS, k_altmin_w ~21 KB: NNQP scratch, k x k work matrices, constraint tables)
#define ALTMIN_KMAX 8
OMC_HD int altmin_variant(int k) { return k == 1 ? 1 : (k <= 4 ? 2 : 3); }
OMC_HD KernelPlan altmin_plan(int n, int m, int k, int Rmax, int nolds) {
  const int var = altmin_variant(k);
  const size_t bytes = (var == 1) ? altmin1_layout(n, m, Rmax).bytes : (var == 2) ? altmink_layout(n, m, k, Rmax).bytes : altminw_layout(n, m, k, Rmax).bytes;
  return plan_block(bytes, bytes + 8 * 1024 <= ((var == 1) ? (size_t)OMC_MAX_DYN_LDS - 8 * 1024 : (size_t)128 * 1024) && !nolds);
}
struct OmcGeom {
  KernelPlan cone, ws, glob, small;       // cone and ws share one slab (cone_scratch) and its stride
  int ws_lpp, ws_rpl2, ws_ld;             // k_cone_ws: lanes per pair (0: order beyond the kernel), rows per lane / 2, leading dimension of G
  size_t cpb_lds_bytes, cpb_slab_lds_bytes, cpb_slab_stride;      // k_colprox_block: dynamic LDS of its two launches, slab doubles per (slot, slab column); set by geom_set_cpblock
  int cp_lds_c, cp_lds_doubles, cp_keepB; // k_colprox: columns up to cp_lds_c rows in LDS (cp_lds_doubles per wave); cp_keepB = 0: dense columns, B is gathered again instead of kept
  size_t cp_scratch_stride, sub_lds;      // k_colprox slab per wave (B*m waves), 0 when every column fits the LDS ; dynamic LDS of k_cone_sub
  int mw; MwLayout mwl;                   // 1: omc_launch_cone_ws takes the multi-workgroup kernels (their slab layout; it shares cone_scratch and its stride)
  int plain_mw;                           // 1: omc_launch_cone takes them for CONE_SEP and CONE_TOPK (omc_launch_cone_plain_mw; mwl is filled, mw may be 0)
};
// switch a planned geometry to the multi-workgroup eigen-kernels at order n: the shared slab grows to their need (a multiple of 4 doubles: 32-byte rows)
OMC_HD void geom_set_mw(OmcGeom& g, int n) {
  g.mw = 1; g.mwl = mw_layout(n);
  size_t st = g.mwl.bytes / 8 + 8; if (st < g.ws.slab_stride) st = g.ws.slab_stride;
  g.cone.slab_stride = g.ws.slab_stride = (st + 3) & ~(size_t)3;
}
// the plain operations on the multi-workgroup kernels at order n: the same layout and the same growth of the shared slab, mw as it is
OMC_HD void geom_set_plain_mw(OmcGeom& g, int n) {
  const int mw = g.mw;
  geom_set_mw(g, n);
  g.mw = mw; g.plain_mw = 1;
}
// k_colprox_block: cl, cs = longest column of its LDS list and of its slab list (0: the list is empty)
OMC_HD void geom_set_cpblock(OmcGeom& g, int cl, int cs) {
  g.cpb_lds_bytes = cl > 0 ? cp_block_layout(cl, 1).doubles * 8 : 0;
  g.cpb_slab_lds_bytes = cs > 0 ? cp_block_layout(cs, 0).doubles * 8 : 0;
  g.cpb_slab_stride = cs > 0 ? cp_block_layout(cs, 0).slab : 0;
}
// n, np16: order of the cone matrix and its padding to 16 (the Shor view of the big cone passes n + m); cmax: longest column;
// cone_multi_min: orders from this value on (and never below MW_MIN_ORDER) take the multi-workgroup eigen-kernels; plain_multi_min: the same
// for the plain operations (a view on which they never run passes a value above MW_MAX_ORDER)
OMC_HD bool mw_order_ok(int n, int use_lds, int knob) { return n >= MW_MIN_ORDER && !use_lds && n >= knob && n <= MW_MAX_ORDER; }
OMC_HD OmcGeom omc_plan_geometry(int n, int np16, int k, int rmax, int Rmax, int cmax, int global_nolds, int cone_multi_min, int plain_multi_min) {
  OmcGeom g;
  const WsGeometry wg = ws_geometry(n);
  g.cone = plan_block(cone_bytes(n), cone_bytes(n) <= OMC_MAX_DYN_LDS);
  g.ws = plan_block(wg.bytes, wg.use_lds != 0);
  g.ws_lpp = wg.lpp; g.ws_rpl2 = wg.rpl >> 1; g.ws_ld = wg.ld;
  g.cone.slab_stride = g.ws.slab_stride = g.cone.slab_stride > g.ws.slab_stride ? g.cone.slab_stride : g.ws.slab_stride;      // one slab serves both: the larger need
  g.sub_lds = sub_layout(np16).bytes;
  const size_t gb = glob_layout(n, k, rmax, Rmax).bytes, sb = small_layout(n, rmax, k).bytes;
  g.glob = plan_block(gb, gb + GLOB_STATIC_LDS <= OMC_MAX_DYN_LDS && !global_nolds);
  g.small = plan_block(sb, sb + SMALL_STATIC_LDS <= OMC_MAX_DYN_LDS);
  g.cp_lds_c = cmax < 64 ? cmax : 64; g.cp_keepB = g.cp_lds_c <= 40 ? 1 : 0;
  g.cp_lds_doubles = cp_reg_layout(g.cp_lds_c, g.cp_keepB).doubles;
  g.cp_scratch_stride = cmax > g.cp_lds_c ? cp_body_layout(cmax).doubles : 0;
  g.mw = g.plain_mw = 0; g.mwl = MwLayout{};
  g.cpb_lds_bytes = g.cpb_slab_lds_bytes = g.cpb_slab_stride = 0;
  if (mw_order_ok(n, wg.use_lds, cone_multi_min)) geom_set_mw(g, n);
  if (mw_order_ok(n, wg.use_lds, plain_multi_min)) geom_set_plain_mw(g, n);
  return g;
}
#endif
