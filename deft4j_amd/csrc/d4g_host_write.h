// d4g_host_write.h — Batch, output side: the bit writer, trailer checksums, the run sequence; round-trip verification.
#pragma once

namespace d4g {

// ---- DeflateStream.write — :128-145 ----
inline void Batch::phase_write() {
    std::vector<D4GWriteJob> jobs;
    i64 words = 0;
    for (HStream& s : streams) {
        s.outWordBase = words;
        if (s.status != 0) continue;
        i64 pos = 0;
        for (size_t k = 0; k < s.blocks.size(); k++) {
            const HBlock& b = s.blocks[k];
            D4GWriteJob j;
            memset(&j, 0, sizeof(j));
            j.blk = b.gpu;
            j.type = b.type;
            j.isFinal = k + 1 == s.blocks.size();
            j.bitStart = words * 32 + pos;
            j.uAbs = s.uBase + b.uStart;
            j.uLen = b.uLen;
            jobs.push_back(j);
            pos += 3;
            pos += b.size_at(pos);
        }
        s.outBits = pos;
        words += (pos + 31) / 32 + 2;
    }
    outWords = words;
    dOut.alloc_zero((size_t)words, 64);
    if (!jobs.empty()) {
        RtScratch tmp;
        D4GWriteJob* dJobs = tmp.upload(jobs);
        D4GCtx c = make_ctx(engine().progDyn, 0);
#ifdef D4G_HOSTSIM
        const int writeBlock = state_block();
#else
        const int writeBlock = 1024;   // one workgroup per block walks its tokens in order: wide steps, few of them
#endif
        RT_LAUNCH(k_write, jobs.size(), writeBlock, c, dJobs, dOut);
        stats.kernel_launches++;
        rt_sync();
        tmp.release();
    }
    check_device_errors();
    for (HStream& s : streams)
        if (s.status == 0) stats.bytes_out += (s.outBits + 7) / 8;
}

// ---- trailer checksums of the decoded bytes (gzip CRC-32 + ISIZE, zlib Adler-32) ----
inline void Batch::checksums() {
    if (!csums.empty() || streams.empty()) return;
    if (!dU) throw std::runtime_error("checksums: the batch has not been parsed");
    RtScratch tmp;
    RtEvent e0, e1;
    e0.record();
    D4GCsumOut* dOutC = launch_checksums(tmp);
    e1.record();
    csums.resize(streams.size());
    rt_d2h(csums.data(), dOutC, streams.size() * sizeof(D4GCsumOut));
    stats.ms_checksum_kernels = rt_elapsed_ms(e0, e1);
    tmp.release();
}
// the two checksum kernels, queued: one record per stream in device memory (`tmp` owns it)
inline D4GCsumOut* Batch::launch_checksums(RtScratch& tmp) {
    size_t n = streams.size();
    std::vector<long long> base(n + 1, 0);
    for (size_t i = 0; i < n; i++) base[i + 1] = base[i] + (streams[i].status == 0 ? (streams[i].nU + D4G_CSUM_TILE - 1) / D4G_CSUM_TILE : 0);
    long long nTiles = base[n];
    long long* dBase = tmp.upload(base);
    D4GCsumRec* dCh = tmp.alloc<D4GCsumRec>((size_t)nTiles, 16);
    D4GCsumOut* dOutC = tmp.alloc<D4GCsumOut>(n);
    if (nTiles) {
        RT_LAUNCH(k_csum_tiles, nTiles, 256, dStreams, dBase, (int)n, dU, engine().dCrcTab, dCh);
        stats.kernel_launches++;
    }
    RT_LAUNCH(k_csum_combine, n, 256, dStreams, dBase, dCh, engine().dCrcTab + 1024, dOutC);
    stats.kernel_launches++;
    return dOutC;
}

inline void Batch::run(bool merge) {
    run_parse(merge);
    run_rest(merge);
}
// no search and no output: the streams' parse and, with `decode`, their decoded bytes (d4g_batch_parse, the one-shot questions, verification)
inline void Batch::parse_only(bool decode) {
    engine().init();
    parse_probe();
    if (decode) build_blocks(false, false);
}
// run() in two steps, for callers that start other work on the decoded bytes between them (the recompress modes)
inline void Batch::run_parse(bool merge) {
    if (ran) throw std::runtime_error("batch already ran");
    ran = true;
    engine().init();
    tRun0 = now_ms();
    parse_probe();
    build_blocks(merge, true);
    tRun1 = now_ms();
}
inline void Batch::run_rest(bool merge) {
    const double t0 = tRun0, t1 = tRun1, t1b = now_ms();   // (other work may have run between the two steps)
    phase1();
    double t2 = now_ms();
    if (merge) phase_merge();
    double t3 = now_ms();
    phase_write();
    double t4 = now_ms();
    stats.ms_parse = t1 - t0;
    stats.ms_optimise = t2 - t1b;
    stats.ms_merge = t3 - t2;
    stats.ms_write = t4 - t3;
    stats.ms_total = (t1 - t0) + (t4 - t1b);
    stats.ms_search_kernels = msSearch;
    stats.ms_parse_kernels = msParseKernels;
    stats.search_bytes_algorithmic = stats.bytes_in + stats.bytes_decoded + stats.bytes_out;
    release_scratch();
}
// After the write phase only the results are needed (output words, decoded bytes, stream table): the search's
// working set goes back to the memory pool, where the next batch finds it.
inline void Batch::release_scratch() {
    rt_sync_all();
    dTok.reset(); dRefs.reset(); dTokRef.reset();
    dBinStat.reset(); dBinMask.reset();
    dHsMemo.reset(); dRcMemo.reset(); dPassMemo.reset();
    dBlocks.reset(); dStates.reset(); dMasks.reset();
    dKeys.reset(); dActive.reset(); dResults.reset();
}

// ---- round-trip verification: the one routine behind d4g_batch_verify, d4g_verify_streams and D4G_VERIFY=1 ----
// An item is (a raw DEFLATE stream, the bytes it must decode to); both live in device memory unless `bytesOnHost`, where
// the stream bytes come from the caller's arrays.  The streams go through the ordinary parse path as one batch of their
// own, then k_verify_compare walks the common prefix of every pair; no decoded byte goes through the host.
enum { VERIFY_OK = 0, VERIFY_SKIPPED = 1, VERIFY_PARSE = -1, VERIFY_SIZE = -2, VERIFY_LENGTH = -3, VERIFY_BYTES = -4 };
struct VerifyItem {
    const uint8_t* bytes = nullptr;   // the stream
    size_t len = 0;
    const uint8_t* want = nullptr;    // expected decoded bytes (device)
    i64 wantLen = 0;
    i64 wantBits = -1;                // >= 0: the parse must read exactly `len` bytes and this many bits
    const uint8_t* dict = nullptr;    // the preset dictionary the stream was written against (its tail, device), as in HStream
    i64 dictLen = 0;
    int verdict = VERIFY_SKIPPED;
    i64 first = -1;
    std::vector<Batch::PBlock> blocks;   // the stream's block list as parsed (empty when it does not parse)
};
struct VerifyTotals { double ms = 0, msKernels = 0; i64 streams = 0, bytes = 0; };

inline void verify_items(std::vector<VerifyItem>& items, bool bytesOnHost, VerifyTotals& T) {
    const size_t n = items.size();
    if (!n) return;
    const double t0 = now_ms();
    std::vector<const uint8_t*> p(n);
    std::vector<size_t> l(n);
    for (size_t i = 0; i < n; i++) { p[i] = items[i].bytes; l[i] = items[i].len; }
    Batch V;
    V.create(n, p.data(), l.data(), !bytesOnHost);
    for (size_t i = 0; i < n; i++) { V.streams[i].dict = items[i].dict; V.streams[i].dictLen = items[i].dictLen; }
    V.parse_only(true);
    std::vector<D4GVerifyPair> pairs;
    std::vector<size_t> owner;
    std::vector<long long> base(1, 0);
    for (size_t i = 0; i < n; i++) {
        VerifyItem& it = items[i];
        const Batch::PStream& P = V.ps[i];
        it.first = -1;
        if (P.status != 0) { it.verdict = VERIFY_PARSE; continue; }
        it.blocks = P.blocks;
        if (it.wantBits >= 0 && (P.consumed != (i64)it.len || P.sizeBits != it.wantBits)) { it.verdict = VERIFY_SIZE; continue; }
        it.verdict = VERIFY_OK;
        const i64 common = std::min(P.nU, it.wantLen);
        T.bytes += common;
        if (common <= 0) continue;
        pairs.push_back({V.dU + V.streams[i].uBase, it.want, common});
        owner.push_back(i);
        base.push_back(base.back() + (common + D4G_CSUM_TILE - 1) / D4G_CSUM_TILE);
    }
    T.streams += (i64)n;
    T.msKernels += V.msParseKernels;
    std::vector<unsigned long long> first(pairs.size(), D4G_VERIFY_NONE);
    if (!pairs.empty()) {
        const size_t np = pairs.size();
        RtScratch tmp;
        D4GVerifyPair* dPairs = tmp.upload(pairs);
        long long* dBase = tmp.upload(base);
        unsigned long long* dFirst = tmp.alloc<unsigned long long>(np);
        rt_memset(dFirst, 0xff, np * 8);
        RtEvent e0, e1;
        e0.record();
        RT_LAUNCH(k_verify_compare, base[np], 256, dPairs, dBase, (int)np, dFirst);
        e1.record();
        rt_d2h(first.data(), dFirst, np * 8);
        T.msKernels += rt_elapsed_ms(e0, e1);
        tmp.release();
    }
    for (size_t k = 0; k < pairs.size(); k++)
        if (first[k] != D4G_VERIFY_NONE) { items[owner[k]].verdict = VERIFY_BYTES; items[owner[k]].first = (i64)first[k]; }
    for (size_t i = 0; i < n; i++) {   // bytes win over length: a difference inside the common prefix is reported as such
        VerifyItem& it = items[i];
        if (it.verdict == VERIFY_OK && V.ps[i].nU != it.wantLen) { it.verdict = VERIFY_LENGTH; it.first = std::min(V.ps[i].nU, it.wantLen); }
    }
    T.ms += now_ms() - t0;
}

}  // namespace d4g
