// d4g_host.h — host orchestration of libdeft4g: the stream-level loops of the reference (DeflateStream.optimise /
// mergeBlocks) and the batch object behind the C ABI.  The host only sequences kernels and resolves the few decisions
// that depend on a stream-wide bit position (stored-block alignment); all token, Huffman and header arithmetic runs in
// the HIP kernels.  This header holds the batch's data; its phases are defined in the d4g_host_*.h headers included at
// the end (parse, search, merge, write), the search program and the per-process engine in d4g_program.h, and every
// environment knob in d4g_knobs.h.  The drivers above a batch have headers of their own: the encoders' front ends (d4g_lz77_host.h,
// d4g_zopfli_host.h), the stream finder (d4g_host_find.h) and CompressionUtil.compress with CMDUtil.optimise's loop (d4g_host_recompress.h).
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <map>
#include <memory>
#include <atomic>
#include <vector>

#include "d4g_ops.h"
#include "d4g_fused.h"
#include "d4g_parse.h"
#include "d4g_rt.h"
#include "d4g_write.h"
#include "d4g_knobs.h"
#include "d4g_program.h"
#include "../../include/deft4g.h"

namespace d4g {

#define D4G_SEG_TARGET_BYTES 8192        // consecutive blocks are gathered into one segment while they decode to no more than this
#define D4G_SEG_MAX_BYTES (1LL << 20)    // D4G_COPY=auto: a block beyond either bound sends its stream the doubling way
#define D4G_SEG_MAX_TOKENS (1LL << 16)
// threads per workgroup of the block-local copy kernels (the emulator's fibers are slow: there, what the block decoders have)
static inline int seg_threads() {
#ifdef D4G_HOSTSIM
    return parse_threads();
#else
    return 1024;
#endif
}

static inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// bytes in device memory; a bit stream's are its whole bytes (a DEFLATE stream ends inside its last byte)
struct DevBytes { const uint8_t* p; size_t len; };
struct DevList { std::vector<const uint8_t*> p; std::vector<size_t> len; void add(DevBytes b) { p.push_back(b.p); len.push_back(b.len); } };   // as the arrays Batch::create takes
static inline DevBytes dev_bits(const uint32_t* words, i64 bits) { return {(const uint8_t*)words, (size_t)((bits + 7) / 8)}; }

// host view of one block of a stream
struct HBlock {
    int type = 0;        // current type (a Huffman block may have become STORED)
    int gpu = -1;        // device block index (Huffman blocks and merge arenas)
    int homeGpu = -1;    // device block of the first parsed block this one covers: where a merged block is committed
    int ordinal = 0;     // that first block's position among the stream's parsed blocks
    i64 tokStart = 0, tokCount = 0, uStart = 0, uLen = 0;
    i64 refStart = 0, refCount = 0;   // back-reference records of the block's tokens
    i64 size = 0;        // Huffman: sizeBits of the current state
    std::vector<D4GRoundResult> chain;  // phase-1 optimiseBlock rounds
    i64 size_at(i64 alignment) const {  // getSizeBits(alignment)
        if (type != D4G_STORED) return size;
        i64 c = alignment % 8;
        c = c == 0 ? 0 : 8 - c;
        return (uLen + 4) * 8 + c;
    }
};

struct HStream {
    int status = 0;
    std::vector<HBlock> blocks;
    i64 consumed = 0, sizeBitsIn = 0, saved = 0;
    i64 inOff = 0, inLen = 0;
    const uint8_t* dict = nullptr;   // preset dictionary: its tail in device memory — the batch's dDict (or that of the batch this one works
                                     // for); an encoder batch's own dU, right in front of the input (LzFront::create).  Both live as long as the batch
    i64 dictLen = 0;                 // bytes of that tail (<= 32768), 0: none
    i64 tokBase = 0, uBase = 0, nTok = 0, nU = 0, refBase = 0, nRef = 0;
    i64 outWordBase = 0, outBits = 0;
    int arena[2] = {-1, -1};
    i64 commitMaskBase = 0;   // mask words where finished merged blocks keep their final mask (see commit_block)
    // mergeBlocks state machine
    size_t mIdx = 0;
    i64 mPos = 0, mSaved = 0;
    bool mFirst = true, mDone = false, mWaiting = false;
    int mArenaUsed = -1;
};

struct Batch {
    struct PBlock { int type, bfinal; i64 bitPos, endBit, nTok, uLen, sizeBits, nRef; int firstBatch; i64 refSpan = -1; i64 hdrBits = 0; int partial = 0; };   // refSpan: records the block occupies in refs even when it is STORED (LZ77 front end); partial: the tokens before a failure (recover), uLen their bytes
    struct PStream {
        int status = 0; std::vector<PBlock> blocks; i64 nTok = 0, nU = 0, consumed = 0, sizeBits = 0; i64 uBaseFixed = -1;   // uBaseFixed: the decoded bytes already sit in U (LZ77 front end: the raw input)
        i64 failBlock = -1, failBit = -1, failU = 0;   // status != 0: the block that did not parse (blocks accepted before it), its first bit, the bytes decoded before it
        std::vector<PBlock> accepted;                  // status != 0: those blocks (`blocks` is empty then), for recover()
    };
    struct ParseError { int reason = 0; i64 block = -1, blockBit = -1, bitPos = -1, decoded = -1, value = -1; };
    struct Layout {     // layout_blocks: the running totals of the per-block arrays and what the emit / copy passes need
        std::vector<int32_t> realBlocks;   // device blocks that come straight from the parse (not merge arenas)
        std::vector<D4GEmitIn> emits;
        std::vector<D4GRecoverIn> partials;   // blocks decoded up to a failure (a recovery's side batch only)
        std::vector<D4GTokRange> ranges;
        int masksAlloc = 1;
        i64 maskWords = 0, binMaskWords = 0, passMemoWords = 0, tokTot = 0, uTot = 0, refTot = 0;
    };
    struct CopyRoute {  // route_streams: which way each stream's decoded bytes are resolved
        std::vector<D4GTokRange> ranges;   // the doubling way: the ranges of its streams
        std::vector<char> doubling;        // per stream: goes that way
        std::vector<D4GSegment> segs;      // the block-local way: segments, their sub-chunks, and per tail slot its index
        std::vector<D4GSubChunk> chunks;   // among the slots of its stream
        std::vector<int32_t> slotOrd;
        i64 maxSlots = 0;
    };
    struct MergeReq { int stream; int arena; };
    struct ChainStart { int32_t stream; i64 bit; i64 dictLen = 0; };   // walk_chains: a block chain begins at this bit of this stream; bytes of preset dictionary before it
    struct BlockMap {   // scan_inputs: the dynamic headers the scan found and the probe confirmed
        std::vector<std::vector<std::pair<i64, int>>> byStream;   // per stream, sorted: bit position -> index in pout
        std::vector<D4GProbeOut> pout;
    };

    // ---- whole batch: lives until the batch is closed ----
    std::vector<std::vector<uint8_t>> inputs;
    std::vector<HStream> streams;
    d4g_stats stats;
    RtBuf<uint8_t> dIn;
    RtBuf<uint8_t> dDict;            // preset dictionaries: the last 32 KiB of each, once per batch (allocated only when there is one)
    std::vector<i64> dictOff, dictTail;   // per dictionary: where its tail starts in dDict, and its length
    RtBuf<uint8_t> dU;               // decoded bytes of every stream
    RtBuf<D4GStreamDesc> dStreams;
    RtBuf<uint32_t> dOut;
    RtBuf<int32_t> dErr;             // device consistency counter of THIS batch (kernels add to it; checked after each phase)
    std::vector<D4GBlock> hBlocks;   // device block descriptors (host copy)
    std::vector<int> gpuType;        // current state type per device block
    std::vector<D4GCsumOut> csums;   // trailer checksums, made on the first question
    i64 outWords = 0, uTotal = 0;
    int slotsAlloc = 0;
    bool ran = false;
    double tRun0 = 0, tRun1 = 0, msSearch = 0, msParseKernels = 0;
    // ---- parse-time: `ps` and the diagnosis stay; the device buffers go back when build_blocks ends ----
    std::vector<PStream> ps;
    std::vector<ParseError> parseErrors;   // why a stream did not parse: one record per stream, made on the first question
    bool diagnosed = false;
    // what decodes before each failed stream's first failure: made on the first question (recover), kept until the batch goes
    bool recovered = false;
    RtBuf<uint8_t> dRecU;                  // the side batch's decoded bytes
    std::vector<i64> recBase, recLen;      // per stream: where its recovered bytes start in dRecU, and how many (parsed streams: 0)
    RtBuf<D4GChunkBatch> dChunkBatches;    // the probe's verified chunk starts, replayed by the emit pass: what chunkPool points to
    RtBuf<unsigned> dChunkNext;
    D4GChunkPool chunkPool = {nullptr, nullptr, 0};
    RtBuf<uint32_t> dSrc;                  // the doubling passes' source positions
    // ---- search scratch: released by release_scratch() after the write phase (all but the last three) ----
    RtBuf<uint2> dTok;
    RtBuf<uint4> dRefs;          // back-reference records
    RtBuf<uint32_t> dTokRef;     // token -> record index
    RtBuf<uint32_t> dBinStat;    // per block: static bin statistics (d4g_types.h)
    RtBuf<uint64_t> dBinMask;    // per block: bin record masks
    RtBuf<D4GBlock> dBlocks;
    RtBuf<D4GState> dStates;
    RtBuf<uint64_t> dMasks;
    RtBuf<int32_t> dActive;
    RtBuf<D4GRoundResult> dResults;
    RtBuf<D4FClArena> dClArena;                  // the cluster kernel's command slots
    std::vector<D4GMergeJob> pendingCommits;     // merged blocks to move out of their arenas (commit_block)
    std::map<int32_t, D4GBlock> blockPatches;    // descriptor changes, applied by one upload + one scatter kernel
    // ---- level executor only: made on its first use (ensure_level_tables) — a batch the fused executor handles alone
    // never allocates or clears them ----
    RtBuf<long long> dKeys;
    RtBuf<D4GHsMemo> dHsMemo;        // per block: header-search memo
    RtBuf<D4GRecodeMemo> dRcMemo;    // per block: Huffman-rebuild memo
    RtBuf<uint64_t> dPassMemo;       // per block: token-pass memo entries
    size_t levelBlocks = 0;
    long long levelPassMemoWords = 0;

    ~Batch() {
        try { rt_sync_all(); } catch (...) {}   // nothing may still be running on a block that goes back to the pool (the members follow)
    }
    int32_t* errors();
    D4GCtx make_ctx(const Program& P, int nActive);
    void check_device_errors();
    // d4g_host_parse.h
    void create(size_t n, const uint8_t* const* in, const size_t* len, bool fromDevice = false);
    void set_dictionaries(size_t nDict, const uint8_t* const* dict, const size_t* dictLen, const int32_t* dictOf);
    D4GStreamDesc stream_desc(size_t i) const;
    bool has_dictionary() const { return stats.dict_streams > 0; }
    void parse_probe();
    void scan_inputs(BlockMap& M);
    void walk_chains(const std::vector<ChainStart>& starts, const BlockMap& M, std::vector<PStream>& out, int maxBlocks);
    void scan_candidates(const uint32_t* dTileStart, unsigned nTiles, i64 totalBytes, std::vector<D4GProbeIn>& cands, std::vector<D4GProbeOut>& pout);
    void diagnose();
    void recover();
    void layout_blocks(bool merge, bool needSlots, Layout& LY);
    int add_block(Layout& LY, bool needSlots, int stream, const HBlock& hb, i64 maskWordsCap, int type);
    void alloc_block_tables(const Layout& LY, bool needSlots);
    void build_blocks(bool merge, bool needSlots);
    CopyRoute route_streams(const std::vector<D4GTokRange>& allRanges, int copyMode) const;
    void copy_block_local(const std::vector<D4GTokRange>& allRanges, const CopyRoute& R, int32_t* dBad, RtScratch& tmp);
    void copy_doubling(const CopyRoute& R, int32_t* dBad, RtScratch& tmp);
    void launch_jump_tiles(const D4GStreamDesc* dStreamsD, const CopyRoute& R, int tileReps, RtScratch& tmp);
    void block_bins(const std::vector<int32_t>& realBlocks, bool needSlots, RtScratch& tmp);
    // d4g_host_search.h
    void ensure_level_tables();
    D4FParams fused_params(int maxRounds, D4GRoundResult* results, int32_t* info);
    void count_state_launch(const int32_t* blk, size_t n);
    std::pair<std::vector<size_t>, std::vector<size_t>> split_for_fused(const std::vector<int>& act) const;
    std::vector<D4GRoundResult> run_round(const std::vector<int>& act);
    bool run_cluster(int blk, D4GRoundResult* out);
    std::vector<std::vector<D4GRoundResult>> run_fused(const std::vector<int>& act, int maxRounds);
    typedef std::vector<std::unique_ptr<RtEvent>> Events;
    std::vector<D4GRoundResult> run_round_levels(const std::vector<int>& act);
    void run_levels_pass(const Program& P, const std::vector<int32_t>& sub, const std::vector<size_t>& subPos, int pass, std::vector<D4GRoundResult>& res);
    static bool stored_wins(const D4GRoundResult& r, i64 uLen, i64 pos, i64* storedSize);
    void phase1();
    // d4g_host_merge.h
    static bool can_merge(const HBlock& a, const HBlock& b);
    bool merge_advance(int si, MergeReq* req);
    void merge_apply(int si, int arena, const D4GRoundResult& r);
    void commit_block(int si, size_t idx);
    void patch_block(int idx);
    void flush_block_patches();
    void flush_commits(D4GMergeJob* dJobs);
    void phase_merge();
    // d4g_host_write.h
    void phase_write();
    void checksums();
    D4GCsumOut* launch_checksums(RtScratch& tmp);
    DevBytes out_bytes(size_t i) const { return dev_bits(dOut + streams[i].outWordBase, streams[i].outBits); }   // stream i as written
    void run(bool merge);
    void parse_only(bool decode);
    void run_parse(bool merge);
    void run_rest(bool merge);
    void release_scratch();
};

inline int32_t* Batch::errors() {
    if (!dErr) dErr.alloc_zero(4);
    return dErr;
}
inline D4GCtx Batch::make_ctx(const Program& P, int nActive) {
    Engine& E = engine();
    D4GCtx c;
    c.tok = dTok; c.refs = dRefs; c.tokRef = dTokRef; c.binStat = dBinStat; c.binMask = dBinMask; c.hsMemo = dHsMemo; c.rcMemo = dRcMemo; c.passMemo = dPassMemo;
    if (!memo_enabled()) { c.hsMemo = nullptr; c.rcMemo = nullptr; c.passMemo = nullptr; }
    c.U = dU; c.blocks = dBlocks; c.states = dStates; c.masks = dMasks;
    c.keys = dKeys; c.ops = P.dOps; c.hdrFlags = E.dHdrTables; c.hdrPrune = E.dHdrTables + 64;
    c.active = dActive; c.errors = errors(); c.opStats = E.dOpStats; c.nActive = nActive; c.nOps = (int)P.ops.size();
    c.slotsPerBlock = slotsAlloc; c.masksPerBlock = E.masksPerBlock;
    return c;
}
inline void Batch::check_device_errors() {
    int32_t e = 0;
    rt_d2h(&e, errors(), 4);
    if (e != 0) {
        rt_memset(errors(), 0, 4);
        rt_sync();
        throw std::runtime_error("device consistency check failed (" + std::to_string(e) + " errors)");
    }
}

}  // namespace d4g

#include "d4g_host_parse.h"
#include "d4g_host_search.h"
#include "d4g_host_merge.h"
#include "d4g_host_write.h"
