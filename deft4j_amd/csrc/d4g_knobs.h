// d4g_knobs.h — every environment variable the library reads, and when it reads it.  Nothing else under csrc calls
// getenv, with one exception: D4G_SIM_LEAST_DIRECT in d4g_ops.h, an emulator-only hook inside device code.
// A knob is read in one of two ways, and the way is part of its contract:
//   knob_now   at every call of its accessor: the tests (and bench.py) switch these between two calls of one process;
//   KNOB_ONCE  at the accessor's first call in the process, and kept: tuning knobs that size launches.
// Each accessor states its default, what it accepts, and what the CPU emulator (D4G_HOSTSIM, tests/hostsim) does instead.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "d4g_ops.h"
#include "d4g_fused.h"
#include "d4g_rt.h"

namespace d4g {

static inline const char* knob_now(const char* name) { return getenv(name); }
static inline int knob_now(const char* name, int def) { const char* t = getenv(name); return t ? atoi(t) : def; }
static inline long long knob_now_ll(const char* name, long long def) { const char* t = getenv(name); return t ? atoll(t) : def; }
#define KNOB_ONCE(name, def) ([] { static const int v = knob_now(name, def); return v; }())
static inline bool knob_is_zero(const char* t) { return t && t[0] == '0'; }   // "0..." switches a default-on feature off

// ---- executors ----
// D4G_EXEC, now.  "fused" (default, also when unset): one workgroup per block runs the whole search out of LDS (d4g_fused.h),
// a lone long block gets the whole device (k_search_cluster), and the level executor (one launch per program level) takes what
// those two hand back: table overflows, cluster refusals, very large merged blocks.  "levels": the level executor runs every
// round — the cross-check.  Anything else throws (a stale environment should be loud): Batch::build_blocks asks before anything is launched.
static inline bool exec_fused() {
    const char* t = knob_now("D4G_EXEC");
    if (!t || !strcmp(t, "fused")) return true;
    if (!strcmp(t, "levels")) return false;
    throw std::runtime_error("D4G_EXEC must be fused or levels");
}
// D4G_FUSED_MAX_REFS, now.  Blocks with more back-references go to the cluster / level executors.  One workgroup per block is
// unbeatable while there are blocks enough to fill the device, but a lone long block is better served by op-level
// parallelism.  Default 2^17 when the round has 8 or more blocks of over 16384 back-references (nLong), else 2^14.
static inline long long fused_max_refs(size_t nLong) { return knob_now_ll("D4G_FUSED_MAX_REFS", nLong >= 8 ? (1LL << 17) : (1LL << 14)); }
// D4G_CLUSTER_MIN_REFS, now (default 2^14): a lone block with more back-references gets the whole device (k_search_cluster).
// D4G_CLUSTER, now: a value starting with 0 = never.
static inline long long cluster_min_refs() { return knob_now_ll("D4G_CLUSTER_MIN_REFS", 1LL << 14); }
static inline bool cluster_enabled() { return !knob_is_zero(knob_now("D4G_CLUSTER")); }
// D4G_CLUSTER_WGS, once: workgroups of the cluster kernel (default: the device's CUs).  Emulator: 3.
static inline int cluster_wgs() {
#ifdef D4G_HOSTSIM
    return 3;
#else
    return KNOB_ONCE("D4G_CLUSTER_WGS", device_cus());
#endif
}
// D4G_STATE_BLOCK, once: threads per state-op workgroup, 64, 128 or 256 (default and fallback 256: four waves per op; with the
// memos a level is bound by its longest ops, not by throughput).  Emulator: D4G_SIM_BLOCK, now and unchecked, goes first
// (fewer fibers to switch between).
static inline int state_block() {
#ifdef D4G_HOSTSIM
    if (const char* e = knob_now("D4G_SIM_BLOCK")) return atoi(e);
#endif
    const int v = KNOB_ONCE("D4G_STATE_BLOCK", 256);
    return v == 64 || v == 128 ? v : 256;
}
// D4G_FUSED_BLOCK, once (default 512): threads per workgroup of the fused executor.  Emulator: state_block(), at least 128
// (the cluster kernel's workgroups are sized the same way there).
static inline int fused_block() {
#ifdef D4G_HOSTSIM
    return std::max(128, state_block());
#else
    return KNOB_ONCE("D4G_FUSED_BLOCK", 512);
#endif
}
// D4G_FUSED_REG_WORDS, now (default 64 * D4F_NWR): mask words the fused kernels keep in registers; the tests lower it to reach
// the LDS path.  D4G_FUSED_STATS, now: set = per-phase accounting into the op statistics (scripts/fused_profile.py).
static inline int fused_reg_words() { return knob_now("D4G_FUSED_REG_WORDS", 64 * D4F_NWR); }
static inline bool fused_stats() { return knob_now("D4G_FUSED_STATS") != nullptr; }
// D4G_FUSED_CAP_MASKS / _CODES / _HDRS, now (defaults D4F_MAXM, D4F_MAXC, D4F_MAXH: the tables' sizes): ids a round of the fused
// and cluster kernels may hand out before it reports a table overflow; the tests lower them to take that exit on small blocks.
// Clamped to [1, D4F_MAXM], [2, D4F_MAXC] (ids 0 and 1 are reserved, and the code table lasts a launch) and [1, D4F_MAXH];
// mask 0 and header 0 are the block's own.  (The code cap bounds the ids a Huffman rebuild is given; d4f_round_setup's reset of a
// nearly full code table, at D4F_MAXC - 32, and the id it gives the incoming code do not look at it.)  D4G_FUSED_CAP_ROUNDS, now (default D4F_MAXROUNDS, clamped to [1, D4F_MAXROUNDS]):
// rounds of a block per launch of k_search_fused, after which a block that still improves is launched again.
static inline int knob_clamped(const char* name, int lo, int hi) { return std::min(std::max(knob_now(name, hi), lo), hi); }
static inline int fused_cap_masks() { return knob_clamped("D4G_FUSED_CAP_MASKS", 1, D4F_MAXM); }
static inline int fused_cap_codes() { return knob_clamped("D4G_FUSED_CAP_CODES", 2, D4F_MAXC); }
static inline int fused_cap_hdrs() { return knob_clamped("D4G_FUSED_CAP_HDRS", 1, D4F_MAXH); }
static inline int fused_cap_rounds() { return knob_clamped("D4G_FUSED_CAP_ROUNDS", 1, D4F_MAXROUNDS); }
// D4G_LANES, now (bench.py's roofline leg sets 1 so that a launch's event time is not inflated by the neighbouring lane):
// block groups of the level executor running concurrently, clamped to 1..RT_MAX_LANES.  Default 2, measured on config 2:
// 1 -> 587, 2 -> 627, 4 -> 494, 8 -> 349 MB/s.
static inline int lanes() { return std::min(std::max(knob_now("D4G_LANES", 2), 1), RT_MAX_LANES); }
// D4G_MEMO, now: a value starting with 0 = every op computes (the run-time memos are an optimisation only).
static inline bool memo_enabled() { return !knob_is_zero(knob_now("D4G_MEMO")); }

// ---- parse ----
// D4G_PARSE_THREADS, now: threads per workgroup of the block decoders (probe / emit / diagnose), that many 512-bit chunks side
// by side: 64, 128, 256 or 512 (default 512; anything else 64).  Emulator: D4G_SIM_PARSE_THREADS instead, default 64.
static inline int parse_threads() {
#ifdef D4G_HOSTSIM
    const int v = knob_now("D4G_SIM_PARSE_THREADS", 64);
#else
    const int v = knob_now("D4G_PARSE_THREADS", 512);
#endif
    return v == 128 || v == 256 || v == 512 ? v : 64;
}
// The bin statistics (k_block_bins, which runs with any workgroup size): compile-time on the GPU, measured in DESIGN §5 — 1024
// threads per workgroup, and up to 4 tiles summed by one workgroup before it adds its table to the block's.  Emulator: the
// block decoders' threads, and D4G_SIM_BINS_SPAN_TILES, now (default the same 4), so that small cases reach a block of several spans.
#ifndef D4G_BINS_THREADS
#define D4G_BINS_THREADS 1024
#endif
#ifndef D4G_BINS_SPAN_TILES
#define D4G_BINS_SPAN_TILES 4
#endif
static inline int bins_threads() {
#ifdef D4G_HOSTSIM
    return parse_threads();
#else
    return D4G_BINS_THREADS;
#endif
}
static inline int bins_span_tiles() {
#ifdef D4G_HOSTSIM
    return std::max(1, knob_now("D4G_SIM_BINS_SPAN_TILES", D4G_BINS_SPAN_TILES));
#else
    return D4G_BINS_SPAN_TILES;
#endif
}
// D4G_COPY, now: how build_blocks resolves the decoded bytes.  "blocks": block-local copies with window markers (k_seg_*);
// "doubling": pointer jumping over the whole stream (k_fill_src / k_jump_* / k_resolve_streams); "auto" (default): blocks,
// except that a stream holding a block one workgroup should not walk alone (more than D4G_SEG_MAX_BYTES decoded bytes or
// D4G_SEG_MAX_TOKENS tokens) goes the doubling way as a whole.  Anything else throws.
enum { D4G_COPY_AUTO = 0, D4G_COPY_DOUBLING = 1, D4G_COPY_BLOCKS = 2 };
static inline int copy_mode() {
    const char* t = knob_now("D4G_COPY");
    if (!t || !strcmp(t, "auto")) return D4G_COPY_AUTO;
    if (!strcmp(t, "doubling")) return D4G_COPY_DOUBLING;
    if (!strcmp(t, "blocks")) return D4G_COPY_BLOCKS;
    throw std::runtime_error("D4G_COPY must be doubling, blocks or auto");
}
// The doubling passes, all once.  D4G_JUMP_STOP_PCT (50): stop doubling once fewer than this share of the bytes still moves.
// D4G_JUMP_TILE_REPS (6): first rounds tile by tile out of the XCDs' L2; 0 = plain rounds only.  D4G_JUMP_THREADS (1024) and
// D4G_JUMP_LDS_KB (70): workgroup size and idle LDS of the tile kernel (not read by the emulator, which launches 256 plain).
static inline int jump_stop_pct() { return KNOB_ONCE("D4G_JUMP_STOP_PCT", 50); }
static inline int jump_tile_reps() { return KNOB_ONCE("D4G_JUMP_TILE_REPS", 6); }
static inline int jump_threads() { return KNOB_ONCE("D4G_JUMP_THREADS", 1024); }
static inline int jump_lds_kb() { return KNOB_ONCE("D4G_JUMP_LDS_KB", 70); }

// ---- the library around the batch ----
// D4G_VERIFY, now: set, non-empty and not exactly "0" = every call that returns rewritten bytes verifies them first.
static inline bool verify_switch() { const char* v = knob_now("D4G_VERIFY"); return v && v[0] && !(v[0] == '0' && !v[1]); }
// D4G_POOL_MAX_MB, at d4g_init: cap of the device-memory pool's held bytes, in MiB; unset = *bytes stays the pool's default.
static inline void pool_max_bytes(size_t* bytes) { if (const char* t = knob_now("D4G_POOL_MAX_MB")) *bytes = (size_t)atoll(t) << 20; }
// D4G_GROUP_BLOCKS, now (default 12000): blocks per recompress group.
static inline long long group_blocks() { return knob_now("D4G_GROUP_BLOCKS", 12000); }
// The Zopfli stage of a recompress group (d4g_host_recompress.h): on the GPU a host thread of its own with low-priority
// streams, started before the other stages; the emulator runs one kernel at a time, so there it runs inline after them.
static inline bool zopfli_stage_threaded() {
#ifdef D4G_HOSTSIM
    return false;
#else
    return true;
#endif
}
// D4G_ZF_TABLE, now: "scan" = Zopfli match table by window scan instead of sorted buckets.  D4G_ZF_POOL_WORDS, now: first size
// of the Zopfli word pool, at least 64 (tests: start small, exercise the growth); 0 here = unset.
static inline bool zf_table_scan() { const char* t = knob_now("D4G_ZF_TABLE"); return t && !strcmp(t, "scan"); }
static inline int zf_pool_words() { const char* t = knob_now("D4G_ZF_POOL_WORDS"); return t ? std::max(64, atoi(t)) : 0; }

// ---- diagnostics on stderr, all now ----
// D4G_DEBUG_ROUNDS, D4G_DEBUG_JUMP: set = one line per search round / per batch of doubling rounds.  D4G_DEBUG_PROGRAM: set =
// the search program's size, 2 or more = its levels too.  D4G_DEBUG_ZOPFLI: 1 = stage times, 2 = per-block phase ticks.
static inline bool debug_rounds() { return knob_now("D4G_DEBUG_ROUNDS") != nullptr; }
static inline bool debug_jump() { return knob_now("D4G_DEBUG_JUMP") != nullptr; }
static inline int debug_program() { const char* t = knob_now("D4G_DEBUG_PROGRAM"); return !t ? 0 : atoi(t) >= 2 ? 2 : 1; }
static inline int debug_zopfli() { return knob_now("D4G_DEBUG_ZOPFLI", 0); }

}  // namespace d4g
