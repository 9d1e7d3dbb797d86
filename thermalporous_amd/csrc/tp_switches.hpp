// thermalporous_hip: the TP_* runtime switches (environment), declared once.  The table below is what the library
// reads, what tp_switch_count / tp_switch_entry report to tools and tests, and what DESIGN.md section 10 lists.
#pragma once
#include <cstdlib>

// X(enumerator suffix, kind, default as documented, when read, effect).  The environment name is "TP_" + suffix.
//   kind: "flag" (unset: the default; set: on iff atoi gives non-zero), "int" or "real" (as parsed; the site maps it)
//   when: "process" (read once, into a static const at the site) or "setup" (read at every preconditioner set-up).
//         TP_DEBUG, a diagnostic, is "process" for its per-call trace (level 2) only: the level 1 lines ask where they print
#define TP_SWITCH_TABLE(X)                                                                                              \
    X(GRAPH, "flag", "1", "process", "0: launch pc_apply eagerly instead of replaying the recorded programs")           \
    X(PIN, "flag", "1", "process", "0: reduction results reach the host by a copy instead of pinned, device-mapped memory") \
    X(FGMRES_PIPE, "flag", "1", "process", "0: FGMRES waits for h before enqueueing the next preconditioner application") \
    X(SPEC_MARGIN, "real", "4", "process", "the speculative application is issued while the extrapolated residual is this many times above the tolerance") \
    X(BCGS_WIDE, "flag", "1", "process", "0: the BiCGStab streaming kernels move one double per item")                  \
    X(MD_CHUNK, "int", "8", "process", "4: entries per lane in the Gram-Schmidt kernels (anything else: 8)")            \
    X(BASIS_VEC, "int", "4", "process", "2 / 1: adjacent floats per load in the Gram-Schmidt kernels on the fp32 basis") \
    X(GS_REVERSE, "flag", "1", "process", "0: the Gram-Schmidt update pass walks front to back like the dot pass")      \
    X(REORTH_DOT_REVERSE, "flag", "0", "process", "1: the second dot pass of ksp_reorth walks the other way")           \
    X(HALO_OVERLAP, "flag", "1", "process", "0: multi-GPU SpMV waits for the halo exchange instead of overlapping it")  \
    X(ASM_LDS, "flag", "0", "process", "1: LDS-tiled assembly kernel")                                                  \
    X(AMG_TAIL_DENSE, "flag", "1", "setup", "0: the tail runs as the multilevel kernel k_amg_tail instead of one dense mat-vec") \
    X(AMG_TAIL_CELLS, "int", "1024", "setup", "levels with at most this many cells run inside the single-workgroup tail") \
    X(AMG_TAIL_LDS, "flag", "1", "setup", "0: the tail keeps its vectors in global memory")                             \
    X(AMG_FUSE_BELOW, "int", "200000", "setup", "levels below this size use the fused residual+restriction / prolongation+sweep kernels") \
    X(AMG_DENSE_MFMA, "flag", "1", "setup", "0: coarsest-grid inverse by the scalar LDS Gauss-Jordan instead of the MFMA one") \
    X(AMG_PAIR, "flag", "1", "process", "0: a smoothed level without pre-sweeps and the pure-transfer level below it transfer in separate launches") \
    X(AMG_RR_FUSE, "flag", "1", "process", "0: k_amg_resid, then k_amg_restrict, instead of k_amg_resid_restrict_tile")  \
    X(AMG_PJ_FUSE, "flag", "1", "process", "0: k_amg_prolong_add, then k_amg_jacobi, instead of k_amg_prolong_jacobi_tile") \
    X(AMG_INVD_LOAD, "flag", "0", "process", "1: the sweeps load omega / diag from the stored plane instead of recomputing it") \
    X(BAMG_TAIL_CELLS, "int", "1024", "setup", "system AMG: first level of the single-workgroup tail")                  \
    X(BAMG_FUSE_BELOW, "int", "200000", "setup", "system AMG: levels below this many cells fuse correction + first post-sweep") \
    X(BAMG_DENSE_LDS, "flag", "1", "process", "0: system AMG's dense inverse in global memory")                         \
    X(ILU_MW, "flag", "1", "process", "0: one-wave ILU(0) sweep kernel instead of the multi-wave one")                  \
    X(ILU_BLOCK, "int", "auto", "process", "1 / 0: grid-layout vectors of the multi-wave sweep moved in blocks of 8 steps (unset: 3-D 1, 2-D 0)") \
    X(ILU_DEPTH, "int", "3", "process", "1: two-buffer prefetch ring in the one-wave ILU solve")                        \
    X(ILU_YLDS, "flag", "1", "process", "0: the ILU solve's intermediate vector goes through HBM even when it fits the LDS") \
    X(ILU1_PACK, "flag", "1", "process", "0: the ILU(1) sweeps stream the padded 64-lane rows instead of the packed copy") \
    X(ILU1_PF, "int", "3", "process", "ILU(1): chunks a sweep keeps in registers (2: one step of loads in flight)")     \
    X(ILU1_FACTOR_TILE, "flag", "1", "process", "0: ILU(1) factorisation with one launch per step instead of one workgroup per tile") \
    X(DEBUG, "int", "0", "process", "1: print the AMG tail layout and the speculation counts (read where they print); 2: also one line per hipGraph call")

enum tp_switch {
#define TP_SWITCH_ENUM(id, kind, dflt, when, effect) TP_SW_##id,
    TP_SWITCH_TABLE(TP_SWITCH_ENUM)
#undef TP_SWITCH_ENUM
    TP_SW_COUNT
};

struct tp_switch_info { const char *name, *kind, *dflt, *when, *effect; };
inline constexpr tp_switch_info tp_switch_infos[TP_SW_COUNT] = {
#define TP_SWITCH_INFO(id, kind, dflt, when, effect) {"TP_" #id, kind, dflt, when, effect},
    TP_SWITCH_TABLE(TP_SWITCH_INFO)
#undef TP_SWITCH_INFO
};

// The accessors read the environment at every call: a site that reads once per process keeps its static const.
inline const char *tp_switch_text(tp_switch s) { return getenv(tp_switch_infos[s].name); }
// unset: the table's default; set: on iff atoi gives non-zero
inline bool tp_switch_flag(tp_switch s) {
    const char *v = tp_switch_text(s);
    return atoi(v ? v : tp_switch_infos[s].dflt) != 0;
}
// as parsed; `unset` is what an unset variable gives (the table's default where that is a number)
inline long tp_switch_int(tp_switch s, long unset) {
    const char *v = tp_switch_text(s);
    return v ? atol(v) : unset;
}
inline long tp_switch_int(tp_switch s) { return tp_switch_int(s, atol(tp_switch_infos[s].dflt)); }
inline double tp_switch_real(tp_switch s, double unset) {
    const char *v = tp_switch_text(s);
    return v ? atof(v) : unset;
}
inline double tp_switch_real(tp_switch s) { return tp_switch_real(s, atof(tp_switch_infos[s].dflt)); }
