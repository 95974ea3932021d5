// d4g_host_recompress.h — the recompression driver: CompressionUtil.compress (every compressor of a mode on every input, each
// output optimised, the smallest kept) and CMDUtil.optimise's per-stream loop around it (recompress the decoded bytes, optimise
// the winner, graft it where it is smaller).  It sequences batches and launches one kernel of its own, the HUFFMAN_ONLY entropy
// bound.  It knows nothing of the C ABI: a refusal is a returned string (as lz_spec_refusal), a failure an exception.
#pragma once
#include <functional>
#include <thread>

#include "d4g_lz77_host.h"
#include "d4g_zopfli_host.h"

namespace d4g {

// compressor list of a recompress mode, in CompressionUtil.getCompressors order (C/CompressionUtil.java:44-78 with the
// flags CMDUtil.java:44-50 derives from the mode)
#define D4G_COMP_JZOPFLI 2   // list entries beyond the two zlib flavours: `strategy` is the option set's index
#define D4G_COMP_CAFE 3
inline std::string mode_refusal(int mode) {   // "" = a mode with a compressor list (NONE has none)
    return mode < D4G_MODE_CHEAP || mode > D4G_MODE_ZOPFLI_VERY_EXTENSIVE ? "mode out of range" : "";
}
inline std::vector<LzSpec> mode_specs(int mode) {
    const std::string why = mode_refusal(mode);
    if (!why.empty()) throw std::runtime_error(why);
    std::vector<LzSpec> list;
    const bool extensive = mode >= D4G_MODE_ZOPFLI_EXTENSIVE;      // Strategy.EXTENSIVE (CMDUtil.java:46)
    for (int st : {LZ_DEFAULT, LZ_FILTERED, LZ_HUFFMAN_ONLY}) list.push_back({0, LZ_FLAVOR_ZLIB, st});       // java (JVM) first (:51-58)
    if (mode >= D4G_MODE_ZOPFLI_VERY_EXTENSIVE)                                                              // jzopfli (:60-62)
        for (int o = 0; o < (extensive ? 5 : 1); o++) list.push_back({0, D4G_COMP_JZOPFLI, o});
    if (mode >= D4G_MODE_ZOPFLI)                                                                             // CafeUndZopfli (:64-66)
        for (int o = 0; o < (extensive ? 3 : 1); o++) list.push_back({0, D4G_COMP_CAFE, o});
    for (int st : {LZ_DEFAULT, LZ_FILTERED, LZ_HUFFMAN_ONLY}) list.push_back({0, LZ_FLAVOR_JZLIB, st});      // jzlib last (:68-75)
    return list;
}
// the option set of a Zopfli list entry: MultiJZopfliCompressor.getOptions (C/MultiJZopfliCompressor.java:18-60: split15/first,
// split15/last, split0/first, split0/last, nosplit; libzopfli's 1000000-byte master block) and
// MultiCafeUndZopfliCompressor.getOptions (C/MultiCafeUndZopfliCompressor.java:19-25,33: FIRST, LAST, NONE; 8 MiB master block)
inline ZfSpec zopfli_options(const LzSpec& e, int input, int iter) {
    ZfSpec z{};
    z.input = input;
    z.iterations = iter < 1 ? 1 : iter;
    if (e.encoder == D4G_COMP_CAFE) {
        z.splitting = e.strategy; z.maxblocks = 15; z.master = 8LL << 20;
    } else {
        static const int split[5] = {ZF_SPLIT_FIRST, ZF_SPLIT_LAST, ZF_SPLIT_FIRST, ZF_SPLIT_LAST, ZF_SPLIT_NONE};
        static const int maxb[5] = {15, 15, 0, 0, 0};
        z.splitting = split[e.strategy]; z.maxblocks = maxb[e.strategy]; z.master = 1000000;
    }
    return z;
}

// Joins its threads on every way out of a scope (a joinable std::thread's destructor calls std::terminate).
struct Joiner {
    std::vector<std::thread> threads;
    void join() {
        for (std::thread& t : threads)
            if (t.joinable()) t.join();
    }
    ~Joiner() { join(); }
};

// ---- d4g_stats of batches that ran one after another for one caller ----
// What adds up: the device's work (launches, rounds, kernel times, bytes moved) and the phases' wall clock.
inline void add_stats(d4g_stats& a, const d4g_stats& o) {
    a.ms_lz_sort += o.ms_lz_sort; a.ms_lz_parse += o.ms_lz_parse; a.ms_lz_emit += o.ms_lz_emit;
    a.lz_parse_passes += o.lz_parse_passes; a.lz_chunks_rerun += o.lz_chunks_rerun; a.lz_symbols += o.lz_symbols;
    a.ms_parse += o.ms_parse; a.ms_optimise += o.ms_optimise; a.ms_merge += o.ms_merge; a.ms_write += o.ms_write;
    a.ms_state_kernels += o.ms_state_kernels; a.state_launches += o.state_launches;
    a.state_tokens_per_round += o.state_tokens_per_round; a.state_bytes_per_round += o.state_bytes_per_round;
    a.kernel_launches += o.kernel_launches; a.rounds += o.rounds; a.n_blocks += o.n_blocks; a.n_tokens += o.n_tokens;
    a.ms_search_kernels += o.ms_search_kernels; a.ms_parse_kernels += o.ms_parse_kernels;
    a.search_bytes_algorithmic += o.search_bytes_algorithmic;
}

// CompressionUtil.compress for inputs that live in host or device memory.  Inputs are processed in groups sized to the
// device memory the candidate search needs (every block owns ~1.6 MB of candidate states); the winners' bytes are kept
// in one device buffer.
struct CompressRun {
    std::vector<int> winner;             // index in list order, per input
    DevList win;                         // its bytes, in dWin
    RtBuf<uint8_t> dWin;
    size_t used = 0;
    d4g_stats agg;                       // add_stats of every stage's batch
    int iter = 20;
    ZfFigures zopfli;
    int64_t outputsOptimised = 0, outputsPruned = 0;
    CompressRun() { memset(&agg, 0, sizeof(agg)); }
};

// A stage of a group: one batch of compressor outputs, and which list entry of which input each of them is — output
// q * entries.size() + k of the batch is list entry entries[k] of the group's input input[q].
struct Stage {
    std::unique_ptr<HostBatch> batch;
    std::vector<int> entries;
    std::vector<size_t> input;
};
struct Best { long long bits = 0; int listIdx = -1; const Batch* owner = nullptr; int stream = -1; };   // the smallest output of an input so far
// A stage that ran is counted, and each of its outputs offered to its input: fewer bits wins, then the lower list index.
inline void take_stage(CompressRun& R, std::vector<Best>& best, const Stage& S) {
    const Batch* owner = &S.batch->impl;
    add_stats(R.agg, owner->stats);
    R.outputsOptimised += (int64_t)owner->streams.size();
    for (size_t st = 0; st < owner->streams.size(); st++) {
        const HStream& s = owner->streams[st];
        const int listIdx = S.entries[st % S.entries.size()];
        // Deft.getSizeBitsFallback of what Deft.optimiseDeflateStream returned: the written optimised stream (a stored
        // block's padding follows its new position) or, when nothing was saved, the input
        const long long bits = s.saved > 0 ? s.outBits : s.sizeBitsIn;
        Best& b = best[S.input[st / S.entries.size()]];
        if (b.listIdx < 0 || bits < b.bits || (bits == b.bits && listIdx < b.listIdx)) b = {bits, listIdx, owner, (int)st};
    }
}
// A zlib-family stage: the entries `entries` of `list` for the inputs `raw` (as many as `input`), one encoder batch.  Made
// first — the inputs are on the device from then on — and run (lz->run) later.
inline Stage lz_stage(const std::vector<LzSpec>& list, const std::vector<int>& entries, const std::vector<size_t>& input, const uint8_t* const* raw,
                      const size_t* len, bool fromDevice) {
    Stage S{std::unique_ptr<HostBatch>(new HostBatch()), entries, input};
    std::vector<LzSpec> specs;
    for (size_t q = 0; q < input.size(); q++)
        for (int k : entries) specs.push_back({(int32_t)q, list[k].encoder, list[k].strategy});
    S.batch->create_encode(input.size(), raw, len, specs.size(), specs.data(), fromDevice);
    return S;
}
// Stage 2: the HUFFMAN_ONLY outputs of the inputs whose entropy bound does not already lose against `best`, run.  The stage
// has no batch when every input is pruned (or the list has no such entry).
inline Stage huffman_stage(CompressRun& R, const LzFront& in, const std::vector<LzSpec>& list, const std::vector<int>& hIdx, const std::vector<Best>& best,
                           bool merge) {
    const size_t n = best.size();
    if (hIdx.empty()) return Stage();
    std::vector<LzBoundJob> jobs;
    for (size_t i = 0; i < n; i++) {
        const DevBytes d = in.input(i);
        for (size_t p = 0; p < d.len; p += LZ_SYMS_PER_BLOCK) jobs.push_back({d.p + p, (int32_t)std::min<size_t>(LZ_SYMS_PER_BLOCK, d.len - p), (int32_t)i});
    }
    std::vector<double> lb(n, 0.0);
    if (!jobs.empty()) {
        RtScratch tmp;
        LzBoundJob* dJ = tmp.upload(jobs);
        double* dLb = tmp.alloc<double>(n, 16);
        rt_memset(dLb, 0, n * 8);
        RT_LAUNCH(k_lz_entropy_bound, jobs.size(), 256, dJ, dLb);
        rt_d2h(lb.data(), dLb, n * 8);
        tmp.release();
    }
    std::vector<size_t> need;
    DevList raw;
    for (size_t i = 0; i < n; i++) {
        const double bound = lb[i] * (1.0 - 1e-9) - 1.0;       // rounding of the sum can only have raised it by less than this
        if (bound > (double)best[i].bits) { R.outputsPruned += (int64_t)hIdx.size(); continue; }
        need.push_back(i);
        raw.add(in.input(i));
    }
    if (need.empty()) return Stage();
    Stage S = lz_stage(list, hIdx, need, raw.p.data(), raw.len.data(), true);
    S.batch->lz->run(true, merge);
    return S;
}
// Stage 3: the Zopfli compressors' outputs, encoded on the device and parsed + optimised like any other stream.  On the GPU it
// runs on its own host thread (its own HIP streams, low priority; zopfli_stage_threaded, d4g_knobs.h): a squeeze keeps a handful
// of waves busy for a long time, and the zlib-family stages fill the rest of the device meanwhile.  It only reads the inputs.
struct ZopfliStage : Stage {
    std::exception_ptr err;   // what the stage threw, for the thread that takes its results
    double ms = 0;            // the encode, up to the start of its outputs' run
    ZfFigures fig;
};
inline void run_zopfli_stage(ZopfliStage& Z, const LzFront& in, const std::vector<LzSpec>& list, int iter, bool merge, int ctx) {
    try {
        rt_ctx() = ctx;   // (a new host thread starts on context 0)
        bind_device();
        const double tz = now_ms();
        const size_t n = Z.input.size();
        std::vector<const uint8_t*> dp(n);
        for (size_t i = 0; i < n; i++) dp[i] = in.input(i).p;
        ZfFront zf;
        zf.create(n, dp.data(), in.rawLen.data());
        std::vector<ZfSpec> zs;
        for (size_t i = 0; i < n; i++)
            for (int k : Z.entries) zs.push_back(zopfli_options(list[k], (int)i, iter));
        zf.encode(zs);
        Z.fig = zf.fig;
        DevList out;
        for (size_t q = 0; q < zs.size(); q++) out.add(zf.out_bytes(q));
        Z.batch.reset(new HostBatch());
        Z.batch->impl.create(zs.size(), out.p.data(), out.len.data(), true);
        Z.ms = now_ms() - tz;
        Z.batch->impl.run(merge);
        zf.release();
    } catch (...) {
        Z.err = std::current_exception();
    }
}
// the winners' bytes go into dWin, device to device
inline void keep_winners(CompressRun& R, size_t i0, const std::vector<Best>& best) {
    for (size_t i = 0; i < best.size(); i++) {
        const DevBytes w = best[i].owner->out_bytes((size_t)best[i].stream);
        R.winner[i0 + i] = best[i].listIdx;
        R.win.p[i0 + i] = R.dWin + R.used;
        R.win.len[i0 + i] = w.len;
        rt_d2d(R.dWin + R.used, w.p, w.len);
        R.used += (w.len + 15) & ~(size_t)15;
    }
    rt_sync();
}
// one group of inputs [i0, i1): the stages, in the order that fills the device best
inline void compress_group(CompressRun& R, size_t i0, size_t i1, const uint8_t* const* raw, const size_t* len, bool fromDevice,
                           const std::vector<LzSpec>& list, bool merge, const std::function<void()>& afterStart) {
    const size_t n = i1 - i0;
    std::vector<int> lzIdx, hIdx, zIdx;   // list positions: outputs that can hold back-references, HUFFMAN_ONLY, the Zopfli entries
    for (size_t k = 0; k < list.size(); k++) {
        if (list[k].encoder >= D4G_COMP_JZOPFLI) zIdx.push_back((int)k);
        else (list[k].strategy == LZ_HUFFMAN_ONLY ? hIdx : lzIdx).push_back((int)k);
    }
    std::vector<size_t> all(n);
    for (size_t i = 0; i < n; i++) all[i] = i;
    Stage S1 = lz_stage(list, lzIdx, all, raw + i0, len + i0, fromDevice);
    const LzFront& in = *S1.batch->lz;   // the group's inputs from here on: they lie in stage 1's dU
    ZopfliStage Z;
    Z.entries = zIdx; Z.input = all;
    const int ctx = rt_ctx();
    const bool threaded = zopfli_stage_threaded();
    Joiner zthread;   // also when a stage below throws
    if (!zIdx.empty() && threaded)
        zthread.threads.emplace_back([&, ctx]() {
            rt_low_priority_thread() = true;      // this thread's streams carry kernels that run for minutes (d4g_rt.h)
            run_zopfli_stage(Z, in, list, R.iter, merge, ctx);
        });
    const double tg0 = now_ms();
    auto tick = [&](const char* what, const Stage* S = nullptr, double msFirst = 0) {   // D4G_DEBUG_ZOPFLI; a stage: its first part / search / merge
        if (debug_zopfli() <= 0) return;
        fprintf(stderr, "[group] +%.1f s: %s", (now_ms() - tg0) / 1000, what);
        if (S && S->batch) fprintf(stderr, " %.1f / %.1f / %.1f s", msFirst / 1000, S->batch->impl.stats.ms_optimise / 1000, S->batch->impl.stats.ms_merge / 1000);
        fprintf(stderr, "\n");
    };
    if (afterStart) afterStart();      // the caller's own work that only had to wait for the Zopfli stage to be under way
    tick("caller's work done");
    S1.batch->lz->run(true, merge);
    tick("zlib-family stage 1 done: front / search / merge", &S1, S1.batch->impl.stats.ms_parse);
    std::vector<Best> best(n);
    take_stage(R, best, S1);
    const Stage S2 = huffman_stage(R, in, list, hIdx, best, merge);
    if (S2.batch) take_stage(R, best, S2);
    if (!zIdx.empty()) {
        tick("stage 2 done, waiting for the Zopfli stage");
        if (threaded) zthread.join();
        else run_zopfli_stage(Z, in, list, R.iter, merge, ctx);
        tick("Zopfli stage done: encode / its outputs' search / merge", &Z, Z.ms);
        if (Z.err) std::rethrow_exception(Z.err);
        for (const HStream& s : Z.batch->impl.streams)
            if (s.status != 0) throw std::runtime_error("zopfli output does not parse");
        R.zopfli += Z.fig;
        take_stage(R, best, Z);
    }
    keep_winners(R, i0, best);
}
inline void compress_run(CompressRun& R, size_t n, const uint8_t* const* raw, const size_t* len, bool fromDevice, int mode, int iter, bool merge,
                         const std::function<void()>& between = nullptr) {
    R.iter = iter;
    int betweenState = 0;      // 0 not run, 1 running, 2 done
    std::function<void()> once = [&]() { if (between && betweenState == 0) { betweenState = 1; between(); betweenState = 2; } };
    const std::vector<LzSpec> list = mode_specs(mode);
    R.winner.assign(n, -1); R.win.p.assign(n, nullptr); R.win.len.assign(n, 0);
    size_t cap = 64;
    for (size_t i = 0; i < n; i++) cap += len[i] + len[i] / 512 + 96;   // a deflate stream never exceeds its input by more than this
    R.dWin.alloc(cap);
    // group size: the candidate search keeps ~1.6 MB of states per block; estimate >= 3 bytes per symbol and let an
    // out-of-memory failure halve the group
    const long long budget = group_blocks();
    size_t i0 = 0;
    long long shrink = 1;
    while (i0 < n) {
        size_t i1 = i0;
        long long est = 0;
        while (i1 < n) {
            long long e = 4 * ((long long)len[i1] / (3LL * LZ_SYMS_PER_BLOCK) + 2);
            if (i1 > i0 && (est + e) * shrink > budget) break;
            est += e;
            i1++;
        }
        try {
            compress_group(R, i0, i1, raw, len, fromDevice, list, merge, once);
            i0 = i1;
        } catch (const std::runtime_error& ex) {
            if (betweenState != 1 && strstr(ex.what(), "hipMalloc") && i1 - i0 > 1) { shrink *= 2; continue; }   // group too large for the device: retry smaller
            throw;
        }
    }
    once();
}

// ---- CMDUtil.optimise's per-stream loop on a batch of deflate streams ----
// What the loop leaves behind: the re-optimised winners of the recompression (its own copy of their bytes) and which streams took them.
struct Recompressed {
    Batch reopt;
    std::vector<int> index;        // stream -> its winner in reopt (-1: the stream did not parse)
    std::vector<int64_t> saved;    // bits the graft saved; 0: the original stays
    explicit Recompressed(size_t n) : index(n, -1), saved(n, 0) {}
    bool grafted(size_t i) const { return saved[i] > 0; }
    DevBytes bytes(size_t i) const { return reopt.out_bytes((size_t)index[i]); }   // of a grafted stream
};
inline std::string recompress_refusal(const Batch& A, int mode) {
    if (mode == D4G_MODE_NONE) return "";
    const std::string why = mode_refusal(mode);
    if (!why.empty() || !A.has_dictionary()) return why;
    return "the batch holds streams with a preset dictionary and the encoders take no dictionary: only mode NONE runs on it";
}
// The stats of the original batch after the loop.  What describes the originals stays its own (streams, blocks, tokens, bytes,
// the phases' wall clock); the device's work in the chained batches — every stage's (R.agg) and the winners' re-optimisation —
// is summed in (add_stats): the same kernels ran, one set of counters; the recompression's own fields are assigned.
inline void fold_recompress_stats(d4g_stats& A, const CompressRun& R, const d4g_stats& reopt, double msEncode, double msReoptimise) {
    const d4g_stats own = A;
    add_stats(A, R.agg);
    add_stats(A, reopt);
    A.ms_parse = own.ms_parse; A.ms_optimise = own.ms_optimise; A.ms_merge = own.ms_merge; A.ms_write = own.ms_write;
    A.n_blocks = own.n_blocks; A.n_tokens = own.n_tokens;
    A.ms_recompress_encode = msEncode;
    A.ms_recompress_encode_front = R.agg.ms_parse;
    A.ms_recompress_encode_search = R.agg.ms_optimise + R.agg.ms_merge;
    A.ms_recompress_reoptimise = msReoptimise;
    A.recompress_outputs = R.outputsOptimised;
    A.recompress_outputs_pruned = R.outputsPruned;
    A.ms_zopfli_table = R.zopfli.msTable; A.ms_zopfli_split = R.zopfli.msSplit; A.ms_zopfli_squeeze = R.zopfli.msSqueeze; A.ms_zopfli_emit = R.zopfli.msEmit;
    A.zopfli_blocks = R.zopfli.blocks; A.zopfli_position_iterations = R.zopfli.positions;
}
// Runs batch A (made by Batch::create, accepted by recompress_refusal) and the loop; nothing is returned when nothing was
// recompressed (mode NONE, or no stream parsed).
inline std::unique_ptr<Recompressed> recompress(Batch& A, int mode, int iter, bool merge) {
    const size_t n = A.streams.size();
    // container.optimise(mergeBlocks) — CMDUtil.java:70.  In a Zopfli mode only the parse happens here: the search of the originals
    // runs once the Zopfli stage of the recompression (its own host thread, a few long-running waves) is under way.
    const bool deferSearch = mode >= D4G_MODE_ZOPFLI;
    A.run_parse(merge);
    if (!deferSearch) A.run_rest(merge);
    // stream.getUncompressedData() -> compUtil.compress(uncompressed, true) — :83-84; the decoded bytes stay in HBM
    std::vector<size_t> ok;
    DevList raw;
    for (size_t i = 0; i < n; i++)
        if (A.streams[i].status == 0) { ok.push_back(i); raw.add({A.dU + A.streams[i].uBase, (size_t)A.streams[i].nU}); }
    if (mode == D4G_MODE_NONE || ok.empty()) { if (deferSearch) A.run_rest(merge); return nullptr; }
    const double tc0 = now_ms();
    CompressRun R;
    compress_run(R, ok.size(), raw.p.data(), raw.len.data(), true, mode, iter, merge, deferSearch ? std::function<void()>([&]() { A.run_rest(merge); }) : std::function<void()>());
    const double t1 = now_ms();
    // new DeflateStream().parse(recompressed); recompStream.optimise(mergeBlocks) — :85-89
    std::unique_ptr<Recompressed> C(new Recompressed(n));
    C->reopt.create(ok.size(), R.win.p.data(), R.win.len.data(), true);
    C->reopt.run(merge);
    for (size_t k = 0; k < ok.size(); k++) {
        C->index[ok[k]] = (int)k;
        if (C->reopt.streams[k].status != 0) continue;                  // recompStream.parse failed: the original stays (:88)
        // recompStream.getSizeBits() / stream.getSizeBits() of the optimised streams (DeflateStream.java:171-182): the
        // written sizes, in which a stored block's padding follows its new position (sizeBitsIn - saved does not)
        const long long recompSize = C->reopt.streams[k].outBits, originalSize = A.streams[ok[k]].outBits;
        if (recompSize < originalSize) C->saved[ok[k]] = originalSize - recompSize;   // the graft, :94-98
    }
    // (the deferred search of the originals ran inside the encode's time and is not the encode's)
    fold_recompress_stats(A.stats, R, C->reopt.stats, t1 - tc0 - (deferSearch ? A.stats.ms_total - A.stats.ms_parse : 0.0), now_ms() - t1);
    return C;
}

}  // namespace d4g
