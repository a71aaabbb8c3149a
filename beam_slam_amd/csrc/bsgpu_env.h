// The BSGPU_* environment switches: the one file of the library that reads the process environment.  docs/SWITCHES.md has the table
// (values, the path each one selects, when the library takes that path by itself, the test that names it).
//
// Nothing here caches: a function reads the environment when it is called.  A switch that is read once per process is a
// `static const` at its caller; a switch a test changes between two solves of one process is read per call / per finalize().
//
// Test hooks — each forces, on a small window, a path the library takes by itself only under another condition:
//   factorisation      CHOL_FUSED CHOL_EXT CHOL_NOTURN SHARED CHAINS POSE_DIAG_LAUNCH NO_LEAF_TILES
//   tile order         DIM_ORDER DIM_ORDER_DEPTH DIM_ABSORB
//   back-substitution  BACKSOLVE_FUSED BACKSOLVE_LEGACY BACKSOLVE_NO_W BACKSOLVE_GLOBAL_Y
//   LM step            GRAPH REDUCE_LAUNCH SCALARS_EVENT UPDATE_SEPARATE CLEAR_AT_START EVAL_MERGE EVAL_SEPARATE MARG_RIDE
//                      LM_AHEAD LM_DEVICE LM_DEVICE_SPLIT NO_GROUP_ASSEMBLY
//   visual tables      FLATTEN PAIRS_BAND BAND_PART PAIR_ENTRIES_SORT NO_CR COMPACT_J
//   inverse depth      IDP_ELIM IDP_GENERIC_ASSEMBLY
//   pose graphs        EXACT_POSE_GRAPH PCG_LAUNCHES PCG_COARSE PCG_GIVE_UP
//   table hand-over    SYNC_FULL SYNC_CHECK
// Log: TIMING.  Timing probes (no alternative path: the same kernels, stamped): CHOL_PROBE BACKSOLVE_PROBE PCG_PROBE.
#pragma once
#include <cstdlib>
#include <cstring>

namespace bsg {

inline const char* env_str(const char* name) { return std::getenv(name); }                                              // the value, or null
inline bool env_set(const char* name) { return std::getenv(name) != nullptr; }                                          // present, whatever the value
inline bool env_zero(const char* name) { const char* e = std::getenv(name); return e && std::atoi(e) == 0; }            // present and 0
inline int env_int(const char* name, int unset) { const char* e = std::getenv(name); return e ? std::atoi(e) : unset; }

// ---- the switches more than one place asks about: one function each, so that the places cannot disagree
inline bool env_timing() { return env_set("BSGPU_TIMING"); }
inline bool env_shared() { return !env_zero("BSGPU_SHARED"); }               // panels of one step may update the same tiles (atomics): on unless =0
inline bool env_chol_fused() { return !env_zero("BSGPU_CHOL_FUSED"); }       // the single-launch factorisation: on unless =0
inline bool env_chol_turns() { return env_zero("BSGPU_CHOL_NOTURN"); }       // =0: updates in turn order (bit-reproducible), and no row segments
inline bool env_backsolve_legacy() { return env_set("BSGPU_BACKSOLVE_LEGACY"); }
inline bool env_backsolve_no_w() { return env_set("BSGPU_BACKSOLVE_NO_W"); }
// -1: not set.  0 or 1 (set to anything): the chain kernels instead of the single-launch forms.  1 (non-zero): their solution vector in global memory.
inline int env_backsolve_global_y() { const char* e = env_str("BSGPU_BACKSOLVE_GLOBAL_Y"); return e ? std::atoi(e) != 0 : -1; }
inline bool env_scalars_event() { return env_set("BSGPU_SCALARS_EVENT"); }
inline bool env_reduce_launch() { return env_set("BSGPU_REDUCE_LAUNCH"); }
inline int env_eval_merge() { return env_int("BSGPU_EVAL_MERGE", 2); }       // the IMU factors in the reprojection launch — 0: never, 1: cost-only passes, 2: both
inline bool env_update_separate() { return env_set("BSGPU_UPDATE_SEPARATE"); }
inline bool env_clear_at_start() { return env_set("BSGPU_CLEAR_AT_START"); }
// (the switches that change which launches a lone step is made of — bsgpu_batch.cpp mirrors the default set only)
inline bool env_step_variants() { return env_set("BSGPU_EVAL_MERGE") || env_scalars_event() || env_update_separate() || env_clear_at_start(); }
inline int env_exact_pose_graph() { const char* e = env_str("BSGPU_EXACT_POSE_GRAPH"); return e ? std::atoi(e) != 0 : -1; }   // -1: not set (the plan's cost decides), 0: never, 1: always
inline bool env_idp_elim() { return !env_zero("BSGPU_IDP_ELIM"); }
inline bool env_flatten_is(const char* where) { const char* e = env_str("BSGPU_FLATTEN"); return e && !std::strcmp(e, where); }   // "host" | "device"

}  // namespace bsg
