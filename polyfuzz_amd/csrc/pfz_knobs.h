// Every environment knob of libpolyfuzz_hip.so: its name, declared once, and the three functions that read the environment.
// The call sites keep their own defaults and clamping.
#pragma once

namespace pfz {

int knob_int(const char *name, int dflt);    // unset or empty: dflt; else atoi
bool knob_set(const char *name);             // the variable exists (whatever it holds)
const char *knob_str(const char *name);      // its text, NULL when unset

namespace knob {

// ---- context (both latched at first use) ----
inline constexpr const char *DEBUG_SYNC = "PFZ_DEBUG_SYNC";    // diagnostic, set = on: synchronise after every profiled kernel -- localise an asynchronous device fault to a kernel
inline constexpr const char *SCAN3 = "PFZ_SCAN3";              // test seam, set = on: the three-kernel scan instead of the single-pass one
// ---- K1 / K2 ----
inline constexpr const char *K1_EXTRACT = "PFZ_K1_EXTRACT";               // test seam: "thread" forces the thread-per-string kernel, "wave" the wave-per-string one; default: by list size
inline constexpr const char *K1_WAVE_STRINGS = "PFZ_K1_WAVE_STRINGS";     // tuning: strings per workgroup of the wave kernel, default 32
inline constexpr const char *K1_TWO_LISTS = "PFZ_K1_TWO_LISTS";           // test seam, A/B: 0 = the second list never in the same launch; default on
inline constexpr const char *K1_FUSE_ROWS = "PFZ_K1_FUSE_ROWS";           // test seam: 0 = two launches (extraction, then the short rows); default fused
inline constexpr const char *NO_LDS_HIST = "PFZ_NO_LDS_HIST";             // test seam, set = on: forces the global-atomics path of huge vocabularies (K1 document frequencies, index build)
inline constexpr const char *K2_SELF_SCAN = "PFZ_K2_SELF_SCAN";           // test seam: 0 = the long-list path on short lists too
// ---- K3 ----
inline constexpr const char *K3_BLOCK = "PFZ_K3_BLOCK";                   // tuning: to-rows per index block, 1024 / 1536 / 2048 / 4096, default 2048
inline constexpr const char *K3_BANK_ORDER = "PFZ_K3_BANK_ORDER";         // test seam: 1 forces the bank-ordering pass of the index build, 0 = never; default: from 32 768 rows
inline constexpr const char *K3_NO_BANK_ORDER = "PFZ_K3_NO_BANK_ORDER";   // A/B, set = on: no bank-ordering pass
inline constexpr const char *K3_SLICES = "PFZ_K3_SLICES";                 // tuning: to-side slices, default 0 = auto
inline constexpr const char *K3_NO_STREAMED = "PFZ_K3_NO_STREAMED";       // test seam, set = on: no streamed (one pass-1 launch) symmetric self-match
inline constexpr const char *K3_LOCKSTEP = "PFZ_K3_LOCKSTEP";             // test seam: 1 = whenever possible, 0 = never; default auto
inline constexpr const char *K3_LS_MIN_TO = "PFZ_K3_LS_MIN_TO";           // tuning: to-rows above which lock-step runs, default 250000
inline constexpr const char *K3_LS_BLOCKS = "PFZ_K3_LS_BLOCKS";           // tuning: blocks per slice, 1 / 2 / 4 / 8, default 4 (4096-row blocks) or 8
inline constexpr const char *K3_LS_WAVES = "PFZ_K3_LS_WAVES";             // tuning: one-wave workgroups per CU, default as many as the LDS holds
inline constexpr const char *K3_LS_CHUNK = "PFZ_K3_LS_CHUNK";             // tuning: rows per pull, default 0 = auto
inline constexpr const char *K3_SYM = "PFZ_K3_SYM";                       // test seam: 0 = never, 1 = whenever the arithmetic allows; default auto
inline constexpr const char *K3_SYM_MIN = "PFZ_K3_SYM_MIN";               // tuning: rows from which the symmetric form runs, default 20480
inline constexpr const char *K3_SYM_FAIL_ALLOC = "PFZ_K3_SYM_FAIL_ALLOC"; // test seam, set = on: the session state's allocation fails (tests of this fallback)
#ifdef PFZ_EXPERIMENTS      // (variant builds only, tools/build_variant.sh -DPFZ_EXPERIMENTS: results wrong on purpose)
inline constexpr const char *K3_ABLATE = "PFZ_K3_ABLATE";                 // timing experiment: 1 = no scatter, 2 = no sweep, 3 = no warm start; default 0
inline constexpr const char *K3_SYM_SOLO = "PFZ_K3_SYM_SOLO";             // timing experiment: "p/N", pass 1 of ONE part of a job cut over N GPUs, alone on this GPU
inline constexpr const char *K7_EXP = "PFZ_K7_EXP";                       // timing experiment: FuzzArgs::exp, default 0
#endif
// ---- K4 ----
inline constexpr const char *K4_FORCE_GENERAL = "PFZ_K4_FORCE_GENERAL";   // test seam, set = on: everything through the general kernel
inline constexpr const char *K4_PARTS = "PFZ_K4_PARTS";                   // test seam, A/B timing: workgroups that share a from-string's to-groups
inline constexpr const char *K4_SIDE_STREAM = "PFZ_K4_SIDE_STREAM";       // A/B, set = on: the classes of long from-strings on the side stream; default off
inline constexpr const char *K4_NO_QUAD = "PFZ_K4_NO_QUAD";               // A/B, set = on: no four-strings-per-wave kernel
inline constexpr const char *K4_NO_OCTO = "PFZ_K4_NO_OCTO";               // A/B, set = on: four strings of <= 32 characters per wave, never eight of <= 16
// ---- K5 ----
inline constexpr const char *K5_PANEL_ROWS = "PFZ_K5_PANEL_ROWS";         // test seam: rows per score panel (several panels on small inputs); default 4 GiB worth
inline constexpr const char *K5_NO_OVERLAP = "PFZ_K5_NO_OVERLAP";         // A/B timing, set = on: no top-n of one panel beside the GEMM of the next
inline constexpr const char *K5_NO_BLOCK_MAX = "PFZ_K5_NO_BLOCK_MAX";     // A/B, test seam, set = on: the row top-n without the GEMM's block maxima
// ---- K7 ----
inline constexpr const char *K7_FORCE_GENERAL = "PFZ_K7_FORCE_GENERAL";   // test seam, set = on: every from-row through the general kernel
inline constexpr const char *K7_PARTS = "PFZ_K7_PARTS";                   // test seam, A/B: workgroups that share a from-string's to-groups, every class
inline constexpr const char *K7_HAND_BATCHES = "PFZ_K7_HAND_BATCHES";     // test seam: hand over early, after this many batches (and without the group minimum)
inline constexpr const char *K7_NO_HANDOVER = "PFZ_K7_NO_HANDOVER";       // A/B, set = on: heavy rows are not handed over to continuation units
inline constexpr const char *K7_ROW_STATS = "PFZ_K7_ROW_STATS";           // diagnostic: a path the per-row counters and phase timers are written to
inline constexpr const char *K7_NO_SIDE_STREAM = "PFZ_K7_NO_SIDE_STREAM"; // A/B, set = on: the classes of long from-strings on the main stream too

}  // namespace knob
}  // namespace pfz
