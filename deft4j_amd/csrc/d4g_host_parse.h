// d4g_host_parse.h — Batch, parse side: upload, header scan and block probes, the block table, decoded bytes, bin statistics.
#pragma once

namespace d4g {

// fromDevice: the `in` pointers are device addresses (another batch's outputs): chained stages stay in HBM
inline void Batch::create(size_t n, const uint8_t* const* in, const size_t* len, bool fromDevice) {
    memset(&stats, 0, sizeof(stats));
    double t0 = now_ms();
    streams.resize(n);
    i64 off = 0;
    for (size_t i = 0; i < n; i++) {
        streams[i].inOff = off;
        streams[i].inLen = (i64)len[i];
        off += ((i64)len[i] + 15) & ~15LL;
        off += 16;
        stats.bytes_in += (i64)len[i];
    }
    i64 total = off + D4G_INCH + 64;   // (the block decoders and the header scan stage whole windows from a stream's last bytes)
    dIn.alloc_zero((size_t)total);
    for (size_t i = 0; i < n; i++) {
        if (fromDevice) rt_d2d(dIn + streams[i].inOff, in[i], len[i]);
        else rt_h2d(dIn + streams[i].inOff, in[i], len[i]);
    }
    rt_sync();
    stats.n_streams = (i64)n;
    stats.ms_upload = now_ms() - t0;
}

// Preset dictionaries (d4g_batch_create_dict): the last 32 KiB of each goes to the device once, however many streams name
// it; a stream's descriptor points at its dictionary's tail.  dictOf == nullptr names none (d4g_find_streams_dict picks
// per candidate).  A dictionary of length 0 is no dictionary; without any, nothing is allocated.  The caller has checked
// the arguments.
inline void Batch::set_dictionaries(size_t nDict, const uint8_t* const* dict, const size_t* dictLen, const int32_t* dictOf) {
    dictOff.assign(nDict, 0);
    dictTail.assign(nDict, 0);
    i64 off = 0;
    for (size_t d = 0; d < nDict; d++) {
        dictTail[d] = (i64)std::min<size_t>(dictLen[d], D4G_WIN);
        dictOff[d] = off;
        off += (dictTail[d] + 15) & ~15LL;
    }
    if (!off) return;
    dDict.alloc_zero((size_t)off);
    for (size_t d = 0; d < nDict; d++)
        if (dictTail[d]) rt_h2d(dDict + dictOff[d], dict[d] + (dictLen[d] - (size_t)dictTail[d]), (size_t)dictTail[d]);
    rt_sync();
    stats.dict_bytes = 0;
    for (size_t d = 0; d < nDict; d++) stats.dict_bytes += dictTail[d];
    for (size_t i = 0; dictOf && i < streams.size(); i++) {
        if (dictOf[i] < 0 || !dictTail[dictOf[i]]) continue;
        streams[i].dict = dDict + dictOff[dictOf[i]];
        streams[i].dictLen = dictTail[dictOf[i]];
        stats.dict_streams++;
    }
}
// stream i as the kernels see it before its decoded bytes have a place
inline D4GStreamDesc Batch::stream_desc(size_t i) const {
    D4GStreamDesc d;
    d.data = dIn ? dIn + streams[i].inOff : nullptr;
    d.len = streams[i].inLen;
    d.uBase = 0;
    d.uLen = 0;
    d.dict = streams[i].dict;
    d.dictLen = streams[i].dictLen;
    return d;
}

// ---- parse: header scan -> block probes -> chain -> emit -> pointer jumping ----
// hit records that come back with the hit count, in one read: up to 45 KB whatever the count turns out to be, the price
// of not waiting for the count first (a batch of config 2 has about 340 hits)
#ifndef D4G_PROBE_HITS_FIRST
#define D4G_PROBE_HITS_FIRST 512
#endif
// Steps 1-2: header scan (one launch: prolog, code-length code, walk over the coded lengths), speculative probes of the
// survivors.  Only the candidates that parse come back, with their probe results; the probe also fills the chunk pool the
// emit pass replays.  dTileStart: per stream the index of its first tile (scan_inputs).
inline void Batch::scan_candidates(const uint32_t* dTileStart, unsigned nTiles, i64 totalBytes, std::vector<D4GProbeIn>& cands, std::vector<D4GProbeOut>& pout) {
    // (every step below ends in a blocking read: a buffer that goes back here is no longer in use)
    // One result buffer: the scan's two counters and the probe's hit count (16 bytes, cleared together), then the hit
    // records, so that one read brings the hit count and the first records.  The survivors are about the streams' blocks;
    // the list is sized for a block per 128 input bytes and made again when a batch holds more.
    const size_t head = 16;
    unsigned cap = (unsigned)std::max<i64>(4096, totalBytes / 128);
    RtBuf<uint8_t> dRes;
    RtBuf<D4GProbeIn> dCands;
    unsigned counts[2] = {0, 0};
    for (int attempt = 0; attempt < 2; attempt++) {
        dCands.alloc((size_t)cap);
        dRes.alloc(head + (size_t)cap * sizeof(D4GProbeHit));
        rt_memset(dRes, 0, head);
        RT_LAUNCH(k_scan_headers, nTiles, 256, dStreams, dTileStart, (unsigned)streams.size(), dCands, (unsigned*)dRes.get(), cap);
        stats.kernel_launches++;
        rt_d2h(counts, dRes, sizeof(counts));
        if (counts[0] <= cap) break;
        cap = counts[0] + 1024;
    }
    // 2. speculative probes of the survivors; only the candidates that parse come back
    const unsigned nc = counts[0];
    stats.scan_candidates = (i64)counts[1];
    stats.scan_kept = (i64)nc;
    if (nc) {
        D4GProbeHit* dHits = (D4GProbeHit*)(dRes.get() + head);
        unsigned* dN = (unsigned*)dRes.get() + 2;
        chunkPool.cap = (unsigned)std::min<i64>(1 << 30, totalBytes * 8 / (64 * D4G_CHUNK_BITS) + 2 * (i64)nc * (parse_threads() / 64) + 64);   // one record per wave and batch
        chunkPool.batches = dChunkBatches.alloc((size_t)chunkPool.cap);
        chunkPool.next = dChunkNext.alloc_zero(4);
        RT_LAUNCH(k_probe_blocks, nc, parse_threads(), dStreams, dCands, (D4GProbeOut*)nullptr, nc, dHits, dN, chunkPool);
        stats.kernel_launches++;
        const size_t first = std::min<size_t>(nc, D4G_PROBE_HITS_FIRST);
        std::vector<uint8_t> back(head + first * sizeof(D4GProbeHit));
        rt_d2h(back.data(), dRes, back.size());
        unsigned nh = 0;
        memcpy(&nh, back.data() + 8, 4);
        std::vector<D4GProbeHit> hits(nh);
        if (nh) memcpy(hits.data(), back.data() + head, std::min<size_t>(nh, first) * sizeof(D4GProbeHit));
        if (nh > first) rt_d2h(hits.data() + first, dHits + first, (nh - first) * sizeof(D4GProbeHit));
        cands.resize(nh);
        pout.resize(nh);
        for (unsigned k = 0; k < nh; k++) { cands[k] = hits[k].in; pout[k] = hits[k].out; }
    }
}

// Steps 1-2 for the batch's inputs: stream table, header scan, and the map of the dynamic headers the probe confirmed
// (per stream: bit position -> probe result), which every chain that crosses the stream shares.
inline void Batch::scan_inputs(BlockMap& M) {
    size_t n = streams.size();
    // the stream table and, behind it in the same upload, where each stream's scan tiles begin (n + 1 entries: a scan
    // workgroup finds its stream there by binary search, so no per-tile table is made or sent)
    const size_t startBytes = (n + 1) * sizeof(uint32_t);
    std::vector<D4GStreamDesc> sd(n + (startBytes + sizeof(D4GStreamDesc) - 1) / sizeof(D4GStreamDesc));
    uint32_t* tileStart = (uint32_t*)(sd.data() + n);
    i64 totalBytes = 0, nTiles = 0;
    for (size_t i = 0; i < n; i++) {
        sd[i] = stream_desc(i);
        tileStart[i] = (uint32_t)nTiles;
        nTiles += (streams[i].inLen + D4G_SCAN_TILE - 1) / D4G_SCAN_TILE;
        if (nTiles > 0x7fffffffLL) throw std::runtime_error("batch holds 2^31 or more scan tiles: split it");
        totalBytes += streams[i].inLen;
    }
    tileStart[n] = (uint32_t)nTiles;
    dStreams.alloc(n, startBytes);
    rt_h2d(dStreams, sd.data(), n * sizeof(D4GStreamDesc) + startBytes);
    std::vector<D4GProbeIn> cands;
    if (nTiles) scan_candidates((const uint32_t*)(dStreams.get() + n), (unsigned)nTiles, totalBytes, cands, M.pout);
    // candidate maps: bit position -> probe result
    M.byStream.assign(n, {});
    for (size_t k = 0; k < cands.size(); k++)
        if (M.pout[k].status == 0) { M.byStream[cands[k].stream].push_back({cands[k].bitPos, (int)k}); stats.scan_confirmed++; }
    for (auto& v : M.byStream) std::sort(v.begin(), v.end());
}

// Host chain walk over chain starts: chain k begins at bit starts[k].bit of stream starts[k].stream and fills out[k] (block
// list, exact token / byte counts; decoded positions and size bits count from the chain's start).  Confirmed headers come
// from the stream's shared map; positions the scan cannot see (fixed / stored / unusual dynamic blocks) are probed
// exactly, the live chains of all streams in one launch per step.  maxBlocks > 0 stops every chain after that many blocks
// (status 0: no block failed so far).
inline void Batch::walk_chains(const std::vector<ChainStart>& starts, const BlockMap& M, std::vector<PStream>& out, int maxBlocks) {
    const size_t n = starts.size();
    out.assign(n, PStream());
    std::vector<i64> cur(n), upos(n, 0), spos(n, 0);
    for (size_t i = 0; i < n; i++) cur[i] = starts[i].bit;
    std::vector<char> done(n, 0);
    RtBuf<D4GProbeIn> dEx;
    RtBuf<D4GProbeOut> dExOut;
    dEx.alloc(n, 16);
    dExOut.alloc(n, 16);
    auto accept = [&](size_t i, i64 bitPos, const D4GProbeOut& o, bool fromScan) {
        PStream& P = out[i];
        if (o.status != 0 || o.needHist > upos[i] + starts[i].dictLen) {
            P.status = -1; done[i] = 1;
            P.failBlock = (i64)P.blocks.size(); P.failBit = bitPos; P.failU = upos[i];
            return;
        }
        P.blocks.push_back({o.type, o.bfinal, bitPos, o.endBit, o.nTok, o.uLen, o.sizeBits, (i64)o.nRef, fromScan ? o.firstBatch : -1, -1, (i64)o.hdrBits});
        upos[i] += o.uLen;
        P.nTok += o.nTok;
        spos[i] += 3;  // DeflateStream.getSizeBits — :171-182
        if (o.type == D4G_STORED) {
            i64 c = spos[i] % 8;
            c = c == 0 ? 0 : 8 - c;
            spos[i] += (o.uLen + 4) * 8 + c;
        } else {
            spos[i] += o.sizeBits;
        }
        cur[i] = o.endBit;
        if (o.bfinal) { done[i] = 1; P.consumed = (o.endBit + 7) / 8; }
        else if (o.eofHit) {   // the next 3-bit read hits EOF
            P.status = -1; done[i] = 1;
            P.failBlock = (i64)P.blocks.size(); P.failBit = o.endBit; P.failU = upos[i];
        }
        else if (maxBlocks > 0 && (int)P.blocks.size() >= maxBlocks) done[i] = 1;
    };
    while (true) {
        std::vector<D4GProbeIn> ex;
        std::vector<size_t> exStream;
        for (size_t i = 0; i < n; i++) {
            while (!done[i]) {
                auto& v = M.byStream[starts[i].stream];
                auto it = std::lower_bound(v.begin(), v.end(), std::make_pair(cur[i], -1));
                if (it != v.end() && it->first == cur[i]) accept(i, cur[i], M.pout[it->second], true);
                else { ex.push_back({starts[i].stream, 0, cur[i]}); exStream.push_back(i); break; }
            }
        }
        if (ex.empty()) break;
        rt_h2d(dEx, ex.data(), ex.size() * sizeof(D4GProbeIn));
        RT_LAUNCH(k_probe_blocks, ex.size(), parse_threads(), dStreams, dEx, dExOut, (unsigned)ex.size(), (D4GProbeHit*)nullptr, (unsigned*)nullptr,
                  D4GChunkPool{nullptr, nullptr, 0u});
        stats.kernel_launches++;
        stats.exact_probes += (i64)ex.size();
        std::vector<D4GProbeOut> eo(ex.size());
        rt_d2h(eo.data(), dExOut, ex.size() * sizeof(D4GProbeOut));
        for (size_t k = 0; k < ex.size(); k++) accept(exStream[k], ex[k].bitPos, eo[k], false);
    }
    dEx.reset(); dExOut.reset();
    for (size_t i = 0; i < n; i++) {
        out[i].nU = upos[i];
        out[i].sizeBits = spos[i];
        if (out[i].status != 0) { out[i].accepted.swap(out[i].blocks); out[i].blocks.clear(); out[i].nTok = 0; out[i].nU = 0; }
    }
}

// Steps 1-2 + host chain walk: fills `ps` (block list per stream, exact token/byte counts) — one chain per stream, from
// its first bit.
inline void Batch::parse_probe() {
    size_t n = streams.size();
    diagnosed = false; parseErrors.clear();   // (answers of an earlier parse go with it)
    recovered = false; dRecU.reset(); recBase.clear(); recLen.clear();
    RtEvent e0, e1;
    e0.record();
    BlockMap M;
    scan_inputs(M);
    std::vector<ChainStart> starts(n);
    for (size_t i = 0; i < n; i++) starts[i] = {(int32_t)i, 0, streams[i].dictLen};
    walk_chains(starts, M, ps, 0);
    e1.record();
    msParseKernels += rt_elapsed_ms(e0, e1);
}

// ---- why a stream did not parse (d4g_batch_parse_error) ----
// One record per stream, made on the first question: a block whose 3 header bits the input no longer holds needs no
// kernel (that covers the empty input and a non-final block that ended it); every other failed stream gets one
// workgroup of a single k_diagnose_blocks launch.  A batch without failed streams launches and allocates nothing.
inline void Batch::diagnose() {
    if (diagnosed) return;
    const size_t n = std::min(ps.size(), streams.size());
    std::vector<ParseError> res(streams.size());
    std::vector<D4GDiagIn> in;
    std::vector<size_t> owner;
    for (size_t i = 0; i < n; i++) {
        const PStream& P = ps[i];
        if (P.status == 0) continue;
        ParseError& e = res[i];
        e.block = P.failBlock; e.blockBit = P.failBit;
        if (P.failBit + 3 > streams[i].inLen * 8) { e.reason = D4G_DIAG_EOF; e.bitPos = P.failBit; e.decoded = P.failU; continue; }
        in.push_back({(int32_t)i, 0, P.failBit, P.failU});
        owner.push_back(i);
    }
    if (!in.empty()) {
        RtScratch tmp;
        D4GDiagIn* dIn2 = tmp.upload(in);
        D4GDiagOut* dOut2 = tmp.alloc<D4GDiagOut>(in.size());
        RT_LAUNCH(k_diagnose_blocks, in.size(), parse_threads(), dStreams, dIn2, dOut2);
        stats.kernel_launches++;
        std::vector<D4GDiagOut> o(in.size());
        rt_d2h(o.data(), dOut2, in.size() * sizeof(D4GDiagOut));
        tmp.release();
        for (size_t k = 0; k < in.size(); k++) {
            if (o[k].reason == D4G_DIAG_OK) throw std::runtime_error("diagnosis: the failing block of stream " + std::to_string(owner[k]) + " decodes");
            ParseError& e = res[owner[k]];
            e.reason = o[k].reason; e.bitPos = o[k].bitPos; e.decoded = o[k].decoded; e.value = o[k].value;
        }
    }
    parseErrors.swap(res);
    diagnosed = true;
}

// ---- what decodes before the first failure (d4g_batch_recover) ----
// The diagnosis says where every failed stream stops: `decoded` bytes into the stream, `decoded - failU` of them in the
// failing block.  A side batch over this batch's device input decodes, per failed stream, the accepted blocks and those
// tokens of the failing block that fit this budget, through the ordinary layout, emit and copy passes; its decoded bytes
// stay here.  Nothing of this batch's own tables is touched, and a batch without failed streams launches and allocates nothing.
inline void Batch::recover() {
    if (recovered) return;
    diagnose();
    const double t0 = now_ms();
    const size_t n = std::min(ps.size(), streams.size());
    std::vector<size_t> owner;
    for (size_t i = 0; i < n; i++) {
        if (ps[i].status == 0 || parseErrors[i].decoded <= 0) continue;
        if (parseErrors[i].decoded >= (1LL << 31)) throw std::runtime_error("recover: stream " + std::to_string(i) + " decodes to 2 GiB or more before its failure");
        if (parseErrors[i].decoded < ps[i].failU) throw std::runtime_error("recover: the diagnosis of stream " + std::to_string(i) + " lies before its failing block");
        owner.push_back(i);
    }
    std::vector<i64> base(streams.size(), 0), len(streams.size(), 0);
    if (owner.empty()) { recBase.swap(base); recLen.swap(len); recovered = true; return; }
    const size_t m = owner.size();
    double msKernels = 0;
    // the failing blocks with a budget: how many tokens and records fit it
    std::vector<D4GRecoverIn> part;
    std::vector<size_t> partOf;
    for (size_t k = 0; k < m; k++) {
        const PStream& P = ps[owner[k]];
        const i64 budget = parseErrors[owner[k]].decoded - P.failU;
        if (budget <= 0) continue;
        D4GRecoverIn ri;
        memset(&ri, 0, sizeof(ri));
        ri.em.stream = (int32_t)owner[k]; ri.em.bitPos = P.failBit; ri.em.firstBatch = -1; ri.budget = budget;
        part.push_back(ri);
        partOf.push_back(k);
    }
    std::vector<D4GProbeOut> cnt(part.size());
    if (!part.empty()) {
        RtScratch tmp;
        RtEvent e0, e1;
        D4GRecoverIn* dPart = tmp.upload(part);
        D4GProbeOut* dCnt = tmp.alloc<D4GProbeOut>(part.size());
        e0.record();
        RT_LAUNCH(k_recover_count, part.size(), parse_threads(), dStreams, dPart, dCnt);
        e1.record();
        stats.kernel_launches++;
        rt_d2h(cnt.data(), dCnt, part.size() * sizeof(D4GProbeOut));
        tmp.release();
        msKernels += rt_elapsed_ms(e0, e1);
        for (size_t q = 0; q < part.size(); q++)
            if (cnt[q].status != 0 || cnt[q].uLen != part[q].budget)   // the diagnosis is the authority: the decode has to meet it
                throw std::runtime_error("recover: the failing block of stream " + std::to_string(owner[partOf[q]]) + " does not decode to the diagnosed offset");
    }
    struct Borrow {   // the input bytes go back to this batch on every way out
        Batch& F; Batch& G;
        Borrow(Batch& F, Batch& G) : F(F), G(G) { G.dIn = std::move(F.dIn); }
        ~Borrow() { try { rt_sync_all(); } catch (...) {} F.dIn = std::move(G.dIn); }
    };
    Batch G;
    memset(&G.stats, 0, sizeof(G.stats));
    Borrow borrow(*this, G);
    G.streams.resize(m);
    G.ps.resize(m);
    for (size_t k = 0; k < m; k++) {
        const PStream& P = ps[owner[k]];
        G.streams[k].inOff = streams[owner[k]].inOff;
        G.streams[k].inLen = streams[owner[k]].inLen;
        G.streams[k].dict = streams[owner[k]].dict;   // (this batch's dDict outlives the side batch)
        G.streams[k].dictLen = streams[owner[k]].dictLen;
        PStream& Q = G.ps[k];
        Q.blocks = P.accepted;
        for (PBlock& pb : Q.blocks) { pb.firstBatch = -1; Q.nTok += pb.nTok; Q.nU += pb.uLen; }   // (the scan's chunk records went back with the parse)
        if (Q.nU != P.failU) throw std::runtime_error("recover: the accepted blocks of stream " + std::to_string(owner[k]) + " do not add up");
    }
    for (size_t q = 0; q < part.size(); q++) {
        PStream& Q = G.ps[partOf[q]];
        PBlock pb = {cnt[q].type, 0, part[q].em.bitPos, 0, cnt[q].nTok, cnt[q].uLen, 0, (i64)cnt[q].nRef, -1};
        pb.partial = 1;
        Q.blocks.push_back(pb);
        Q.nTok += pb.nTok;
        Q.nU += pb.uLen;
    }
    G.build_blocks(false, false);
    msKernels += G.msParseKernels;
    for (size_t k = 0; k < m; k++) { base[owner[k]] = G.streams[k].uBase; len[owner[k]] = G.streams[k].nU; stats.recover_bytes += G.streams[k].nU; }
    dRecU = std::move(G.dU);
    recBase.swap(base); recLen.swap(len);
    recovered = true;
    stats.kernel_launches += G.stats.kernel_launches;
    stats.recover_streams += (i64)m;
    stats.ms_recover_kernels += msKernels;
    stats.ms_recover += now_ms() - t0;
}

// ---- device block table: host block lists, device descriptors and every per-block array, from `ps` ----
// one device block (a parsed Huffman block, or a merge arena): its descriptor and its share of every per-block array
inline int Batch::add_block(Layout& LY, bool needSlots, int stream, const HBlock& hb, i64 maskWordsCap, int type) {
    D4GBlock b;
    memset(&b, 0, sizeof(b));
    b.type = type;
    b.stream = stream;
    b.tokStart = hb.tokStart;
    b.tokCount = hb.tokCount;
    b.uBase = streams[stream].uBase;
    b.uStart = hb.uStart;
    b.uLen = hb.uLen;
    b.stateIdx = (i64)hBlocks.size() * slotsAlloc;
    b.maskBase = LY.maskWords;
    b.maskWords = (hb.refCount + 63) / 64;
    b.refStart = hb.refStart;
    b.refCount = hb.refCount;
    b.binStat = needSlots ? (i64)hBlocks.size() * D4G_NBINS * D4G_BINSTRIDE : -1;
    b.binMask = LY.binMaskWords;
    if (needSlots) LY.binMaskWords += (i64)D4G_NBINS * maskWordsCap;
    b.passMemo = needSlots ? LY.passMemoWords : -1;
    b.passMemoStride = D4G_PASSMEMO_HDR_WORDS + 2 * maskWordsCap;   // header + key codes, outgoing mask, incoming mask (key)
    if (needSlots) LY.passMemoWords += (i64)D4G_PASSMEMO_SLOTS * b.passMemoStride;
    LY.maskWords += maskWordsCap * LY.masksAlloc;
    hBlocks.push_back(b);
    gpuType.push_back(type);
    return (int)hBlocks.size() - 1;
}
inline void Batch::layout_blocks(bool merge, bool needSlots, Layout& LY) {
    Engine& E = engine();
    size_t n = streams.size();
    slotsAlloc = needSlots ? E.slotsPerBlock : 1;
    LY.masksAlloc = needSlots ? E.masksPerBlock : 1;
    hBlocks.clear();
    gpuType.clear();
    i64 &maskWordsTotal = LY.maskWords, &binMaskWords = LY.binMaskWords, &tokTot = LY.tokTot, &uTot = LY.uTot, &refTot = LY.refTot;
    std::vector<D4GStreamDesc> sd(n);
    for (size_t si = 0; si < n; si++) {
        HStream& s = streams[si];
        const PStream& P = ps[si];
        s.status = P.status;
        s.consumed = P.consumed;
        s.sizeBitsIn = P.sizeBits;
        s.nTok = P.nTok;
        s.nU = P.nU;
        s.tokBase = tokTot;
        s.refBase = refTot;
        s.uBase = P.uBaseFixed >= 0 ? P.uBaseFixed : uTot;
        sd[si] = stream_desc(si);
        sd[si].uBase = s.uBase;
        sd[si].uLen = P.nU;
        tokTot += P.nTok;
        if (P.uBaseFixed < 0) uTot += (P.nU + 15) & ~15LL;
        if (P.status != 0) continue;
        int nHuff = 0;
        i64 tpos = 0, upos = 0, rpos = 0;
        for (const PBlock& pb : P.blocks) {
            HBlock hb;
            hb.type = pb.type;
            hb.tokStart = s.tokBase + tpos;
            hb.tokCount = pb.nTok;
            hb.uStart = upos;
            hb.uLen = pb.uLen;
            hb.refStart = s.refBase + rpos;
            hb.refCount = pb.type == D4G_STORED ? 0 : pb.nRef;
            hb.size = pb.sizeBits;
            D4GEmitIn em;
            memset(&em, 0, sizeof(em));
            em.stream = (int32_t)si;
            em.type = pb.type;
            em.bitPos = pb.bitPos;
            em.tokStart = hb.tokStart;
            em.uStart = upos;
            em.uLen = pb.uLen;
            em.stateIdx = -1;
            em.sizeBits = pb.sizeBits;
            em.refStart = hb.refStart;
            em.firstBatch = pb.firstBatch;
            if (pb.type != D4G_STORED) {
                hb.gpu = add_block(LY, needSlots, (int)si, hb, (hb.refCount + 63) / 64, pb.type);
                em.stateIdx = hBlocks[hb.gpu].stateIdx;
                hb.homeGpu = hb.gpu;
                LY.realBlocks.push_back(hb.gpu);
                nHuff++;
            }
            hb.ordinal = (int)s.blocks.size();
            if (pb.partial) LY.partials.push_back({em, pb.uLen, pb.nTok, pb.nRef});
            else LY.emits.push_back(em);
            LY.ranges.push_back({(int32_t)si, pb.type == D4G_STORED ? 1 : 0, hb.tokStart, hb.tokCount, upos, pb.uLen});
            s.blocks.push_back(hb);
            tpos += pb.nTok;
            upos += pb.uLen;
            rpos += pb.refSpan >= 0 ? pb.refSpan : hb.refCount;
            stats.n_blocks++;
        }
        s.nRef = rpos;
        refTot += rpos;
        stats.n_tokens += P.nTok;
        stats.bytes_decoded += P.nU;
        if (merge && needSlots && nHuff >= 2) {
            // (mask slots of an arena start on 128-byte lines and are whole lines long: the cluster kernel's workgroups hand
            // mask words to each other and must never share a line between a slot already read and one still to be written)
            HBlock empty;
            empty.tokStart = s.tokBase;
            empty.refStart = s.refBase;
            for (int a = 0; a < 2; a++) {
                maskWordsTotal = (maskWordsTotal + 15) & ~15LL;
                binMaskWords = (binMaskWords + 15) & ~15LL;
                s.arena[a] = add_block(LY, needSlots, (int)si, empty, (((s.nRef + 63) / 64 + 1) + 15) & ~15LL, D4G_FIXED);
            }
            // a finished merged block moves out of its arena (the two arenas are re-used by the next chain of merges)
            s.commitMaskBase = maskWordsTotal;
            maskWordsTotal += (s.nRef + 63) / 64 + (i64)P.blocks.size() + 2;
        }
    }
    if (!dStreams) dStreams.alloc(n, 16);
    rt_h2d(dStreams, sd.data(), n * sizeof(D4GStreamDesc));
    if (refTot >= (1LL << 32)) throw std::runtime_error("batch holds 2^32 or more back-references: split it");
    uTotal = uTot;
    alloc_block_tables(LY, needSlots);
}
// the token, record and byte arrays and every per-block array, sized by layout_blocks
inline void Batch::alloc_block_tables(const Layout& LY, bool needSlots) {
    const size_t nb = hBlocks.size();
    // (the LZ77 front end has filled tok / refs / tokRef / U already, with the same numbering)
    if (!dTok) dTok.alloc((size_t)LY.tokTot, 64);
    if (!dRefs) dRefs.alloc((size_t)LY.refTot, 64);
    if (!dTokRef) dTokRef.alloc((size_t)LY.tokTot, 64);
    if (!dU) dU.alloc((size_t)LY.uTot, 64);
    if (!nb) return;
    dBlocks.alloc(nb);
    rt_h2d(dBlocks, hBlocks.data(), nb * sizeof(D4GBlock));
    dStates.alloc(nb * (size_t)slotsAlloc);
    dMasks.alloc((size_t)LY.maskWords, 64);
    levelBlocks = needSlots ? nb : 0;
    levelPassMemoWords = LY.passMemoWords;
    if (needSlots && !exec_fused()) ensure_level_tables();   // (the fused executor's batches make them when a block first falls back)
    dActive.alloc(nb);
    dResults.alloc(nb);
    // mask 0 of every block starts empty (no back-reference expanded); the writer reads it even when no search runs
    rt_memset(dMasks, 0, (size_t)LY.maskWords * 8 + 64);   // one fill instead of one per block
    if (needSlots) {
        dBinStat.alloc_zero(nb * (size_t)D4G_NBINS * D4G_BINSTRIDE);
        dBinMask.alloc_zero((size_t)LY.binMaskWords, 64);
    }
}

// ---- steps 3-5 of the parse: emit tokens/states, resolve decoded bytes, bin statistics ----
inline void Batch::build_blocks(bool merge, bool needSlots) {
    const size_t n = streams.size();
    i64 maxU = 0;
    for (size_t i = 0; i < n; i++) maxU = std::max(maxU, ps[i].nU);
    if (maxU >= (1LL << 31)) throw std::runtime_error("a stream decodes to 2 GiB or more");   // (k_fill_src's positions would reach D4G_SRC_FINAL)
    Layout LY;
    layout_blocks(merge, needSlots, LY);
    (void)exec_fused();   // an unknown D4G_EXEC is refused here, where copy_mode() refuses an unknown D4G_COPY: nothing is in flight yet
    const CopyRoute R = route_streams(LY.ranges, copy_mode());
    if (!R.ranges.empty()) dSrc.alloc((size_t)uTotal, 64);
    RtEvent e0, e1;
    e0.record();
    int32_t* dBad = nullptr;          // per stream: a back-reference reached before the start of the stream
    RtScratch tmp;                    // device buffers the queued kernels still read: released after the wait below
    if (!LY.emits.empty() || !LY.partials.empty()) {
        // 3. emit
        D4GParseOut po = {dTok, dU, dStates, dRefs, dTokRef};
        if (!LY.emits.empty()) {
            D4GEmitIn* dEm = tmp.upload(LY.emits);
            RT_LAUNCH(k_emit_blocks, LY.emits.size(), parse_threads(), dStreams, dEm, po, errors(), chunkPool);
            stats.kernel_launches++;
        }
        if (!LY.partials.empty()) {
            D4GRecoverIn* dPart = tmp.upload(LY.partials);
            RT_LAUNCH(k_recover_emit, LY.partials.size(), parse_threads(), dStreams, dPart, po, errors());
            stats.kernel_launches++;
        }
        // 4. decoded bytes (no wait in here: the bin statistics follow on the same stream; the flags come back behind them, one wait for both)
        dBad = tmp.alloc_zero<int32_t>(n, 16);
        if (!R.segs.empty()) copy_block_local(LY.ranges, R, dBad, tmp);
        if (!R.ranges.empty()) copy_doubling(R, dBad, tmp);
    }
    block_bins(LY.realBlocks, needSlots, tmp);
    e1.record();
    if (dBad) {
        std::vector<int32_t> bad(n);
        rt_d2h(bad.data(), dBad, n * 4);
        tmp.release();
        for (size_t i = 0; i < n; i++)
            if (bad[i]) throw std::runtime_error("parse: back-reference before the start of stream (host check missed it)");
    } else {
        rt_sync();
        tmp.release();
    }
    msParseKernels += rt_elapsed_ms(e0, e1);
    dSrc.reset();
    dChunkBatches.reset(); dChunkNext.reset();
    chunkPool = {nullptr, nullptr, 0};
    check_device_errors();
}
// Routes every stream (host only, launches nothing): segments, tail slots and sub-chunks for the block-local copy, or its
// ranges for the doubling passes.
inline Batch::CopyRoute Batch::route_streams(const std::vector<D4GTokRange>& allRanges, int copyMode) const {
    CopyRoute R;
    R.doubling.assign(streams.size(), 0);
    for (size_t i = 0; i < allRanges.size();) {
        size_t j = i;
        const int32_t si = allRanges[i].stream;
        bool old = copyMode == D4G_COPY_DOUBLING;
        for (; j < allRanges.size() && allRanges[j].stream == si; j++)
            if (copyMode == D4G_COPY_AUTO && (allRanges[j].uLen > D4G_SEG_MAX_BYTES || allRanges[j].tokCount > D4G_SEG_MAX_TOKENS)) old = true;
        if (old) {
            R.doubling[si] = 1;
            R.ranges.insert(R.ranges.end(), allRanges.begin() + i, allRanges.begin() + j);
        } else {
            std::vector<D4GSegment>& segs = R.segs;
            const size_t first = segs.size();
            for (size_t k = i; k < j;) {
                size_t e = k + 1;
                i64 bytes = allRanges[k].uLen;
                while (e < j && bytes + allRanges[e].uLen <= D4G_SEG_TARGET_BYTES) bytes += allRanges[e++].uLen;
                segs.push_back({si, (int32_t)k, (int32_t)(e - k), -1, -1, 0, allRanges[k].uStart, bytes});
                k = e;
            }
            // the tail of every segment but the last is the window of the next one
            for (size_t q = first; q + 1 < segs.size(); q++) {
                segs[q].tail = (int32_t)R.slotOrd.size();
                segs[q + 1].win = segs[q].tail;
                R.slotOrd.push_back((int32_t)(q - first));
            }
            R.maxSlots = std::max(R.maxSlots, (i64)(segs.size() - first) - 1);
            for (size_t q = first; q < segs.size(); q++)
                for (i64 o = 0; o < segs[q].uLen; o += D4G_SUB_CHUNK)
                    R.chunks.push_back({si, segs[q].win, segs[q].uStart + o, std::min<i64>(D4G_SUB_CHUNK, segs[q].uLen - o)});
        }
        i = j;
    }
    return R;
}
// The block-local way: symbols per segment, compose rounds over the tail windows, substitute per sub-chunk.
inline void Batch::copy_block_local(const std::vector<D4GTokRange>& allRanges, const CopyRoute& R, int32_t* dBad, RtScratch& tmp) {
    D4GTokRange* dAll = tmp.upload(allRanges);
    D4GSegment* dSegs = tmp.upload(R.segs);
    uint16_t* dSym = tmp.alloc<uint16_t>((size_t)uTotal, 64);
    const size_t slots = R.slotOrd.size();
    uint16_t* dTailA = slots ? tmp.alloc<uint16_t>(slots * D4G_WIN) : nullptr;
    bool anyDict = false;   // (a side batch borrows its streams' dictionaries: ask the streams, not dDict)
    for (const HStream& s : streams) anyDict |= s.dictLen > 0;
    if (anyDict) RT_LAUNCH(k_seg_symbols<true>, R.segs.size(), seg_threads(), dStreams, dSegs, dAll, dTok, dU, dSym, dTailA, dBad);
    else RT_LAUNCH(k_seg_symbols<false>, R.segs.size(), seg_threads(), dStreams, dSegs, dAll, dTok, dU, dSym, dTailA, dBad);
    stats.kernel_launches++;
    stats.copy_segments += (i64)R.segs.size();
    // windows: rounds of the scan are sized from the segment counts, nothing is read back
    if (R.maxSlots > 1) {
        int32_t* dOrd = tmp.upload(R.slotOrd);
        uint16_t* dTailB = tmp.alloc<uint16_t>(slots * D4G_WIN);
        const int GC = 4;
        for (i64 d = 1; d < R.maxSlots; d <<= 1) {
            RT_LAUNCH(k_seg_compose, slots * GC, 256, dOrd, dTailA, dTailB, (int)d, GC);
            std::swap(dTailA, dTailB);
            stats.kernel_launches++;
            stats.copy_rounds++;
        }
    }
    if (!R.chunks.empty()) {
        D4GSubChunk* dChunks = tmp.upload(R.chunks);
        RT_LAUNCH(k_seg_substitute, R.chunks.size(), seg_threads(), dStreams, dChunks, dSym, dTailA, dU);
        stats.kernel_launches++;
    }
}
#ifndef D4G_HOSTSIM
// more than 64 KiB of dynamic LDS has to be allowed once per device
static inline void allow_jump_tile_lds(int kb) {
    static std::atomic<unsigned long long> allowed{0};
    int dev = 0;
    RT_CHECK(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (allowed.load() & bit) return;
    RT_CHECK(hipFuncSetAttribute((const void*)k_jump_tiles, hipFuncAttributeMaxDynamicSharedMemorySize, kb * 1024));
    allowed.fetch_or(bit);
}
#endif
// consecutive tiles -> workgroup ids equal mod 8 (one XCD, one L2): region x of the tile list goes to ids x, x + 8, ...
static inline std::vector<D4GJumpTile> xcd_order(const std::vector<D4GJumpTile>& tl) {
    const size_t nt = tl.size(), per = (nt + 7) / 8;
    std::vector<D4GJumpTile> ord(nt);
    size_t w = 0;
    for (size_t j = 0; j < per; j++)
        for (size_t x = 0; x < 8; x++) {
            const size_t t = x * per + j;
            if (t < nt) ord[w++] = tl[t];
        }
    return ord;
}
// the first doubling rounds tile by tile, out of the XCDs' L2 (k_jump_tiles)
inline void Batch::launch_jump_tiles(const D4GStreamDesc* dStreamsD, const CopyRoute& R, int tileReps, RtScratch& tmp) {
    std::vector<D4GJumpTile> tl;
    for (size_t i = 0; i < streams.size(); i++)
        for (i64 q = 0; R.doubling[i] && q < ps[i].nU; q += D4G_JUMP_TILE) tl.push_back({(int32_t)i, 0, q});
    if (tl.empty()) return;
    const size_t nt = tl.size();
    D4GJumpTile* dTl = tmp.upload(xcd_order(tl));   // (released with the other parse buffers, after the next wait)
    unsigned long long* dCh0 = tmp.alloc_zero<unsigned long long>(2);
#ifdef D4G_HOSTSIM
    RT_LAUNCH(k_jump_tiles, nt, 256, dStreamsD, dTl, dSrc, tileReps, dCh0);
#else
    // 1024 threads per tile and 70 KiB of LDS the kernel never touches: at most two tiles per CU (one beside a resident
    // search workgroup), so the tiles of an XCD's CUs and their neighbours stay in its L2 over the rounds (2.89 -> 2.66 ms
    // of parse kernels at one tile per CU, 100 KiB; 70 KiB is what several batches in flight like best: 12.5-13.0 ->
    // 13.3-13.4 GB/s on config 2)
    const int jt = jump_threads(), jl = jump_lds_kb();
    if (jl > 64) allow_jump_tile_lds(jl);
    hipLaunchKernelGGL(k_jump_tiles, dim3((unsigned)nt), dim3((unsigned)jt), (size_t)jl * 1024, rt().sa(), dStreamsD, dTl, dSrc, tileReps, dCh0);
    RT_CHECK(hipGetLastError());
#endif
    stats.kernel_launches++;
}
// The doubling way: fill the source positions, tile rounds, plain rounds until few bytes still move, resolve.
inline void Batch::copy_doubling(const CopyRoute& R, int32_t* dBad, RtScratch& tmp) {
    const size_t n = streams.size();
    // (the passes go stream by stream: when other streams go the block-local way they get a stream table in which those are empty)
    const D4GStreamDesc* dStreamsD = dStreams;
    std::vector<D4GStreamDesc> sd;
    if (!R.segs.empty()) {
        sd.resize(n);
        for (size_t i = 0; i < n; i++) { sd[i] = stream_desc(i); sd[i].uBase = streams[i].uBase; sd[i].uLen = R.doubling[i] ? ps[i].nU : 0; }
        dStreamsD = tmp.upload(sd);
    }
    i64 maxDoubling = 0, totalU = 0;
    for (size_t i = 0; i < n; i++)
        if (R.doubling[i]) { maxDoubling = std::max(maxDoubling, ps[i].nU); totalU += ps[i].nU; }
    D4GTokRange* dRanges = tmp.upload(R.ranges);
    const int GF = 8;
    RT_LAUNCH(k_fill_src, R.ranges.size() * GF, 256, dStreamsD, dRanges, dTok, dU, dSrc, dBad, GF);
    stats.kernel_launches++;
    const int G = (int)std::min<i64>(2048, std::max<i64>(1, (maxDoubling + 4095) / 4096));
    unsigned long long* dChanged = tmp.alloc_zero<unsigned long long>(40);   // one counter per round, zeroed once
    const unsigned long long stopNum = std::max<unsigned long long>(1, (unsigned long long)((totalU * jump_stop_pct() + 99) / 100));   // the resolve pass walks what is left of the chains
    const int tileReps = jump_tile_reps();
    if (tileReps > 0) launch_jump_tiles(dStreamsD, R, tileReps, tmp);
    const int JB = tileReps > 0 ? 4 : 10;   // rounds per batch: launched back to back, counters read once (after the tile rounds one or two are left)
    for (int base = 0; base < 40; base += JB) {
        for (int round = base; round < base + JB; round++) {
            RT_LAUNCH(k_jump_streams, n * (size_t)G, 256, dStreamsD, dSrc, dChanged + round, G,
                      round == 0 ? (const unsigned long long*)nullptr : dChanged + round - 1, stopNum);
            stats.kernel_launches++;
        }
        unsigned long long ch[10];
        rt_d2h(ch, dChanged + base, JB * 8);
        if (debug_jump()) {
            fprintf(stderr, "jump rounds %d..%d of %lld bytes, moved:", base, base + JB - 1, (long long)totalU);
            for (int k = 0; k < JB; k++) fprintf(stderr, " %llu", ch[k]);
            fprintf(stderr, "\n");
        }
        bool done = false;
        for (int k = 0; k < JB; k++) {
            stats.jump_rounds++;                   // round base + k ran (its predecessor moved enough)
            if (ch[k] < stopNum) { done = true; break; }
        }
        if (done) break;
    }
    RT_LAUNCH(k_resolve_streams, n * (size_t)G, 256, dStreamsD, dSrc, dU, G);
    stats.kernel_launches++;
}
// 5. static bin statistics of every block's back-reference records (the least-expensive pass works from them);
//    also fills in the records' first decoded bytes
// (queued, not waited for: the block list comes from the caller's scratch, released after its next wait on the stream)
inline void Batch::block_bins(const std::vector<int32_t>& realBlocks, bool needSlots, RtScratch& tmp) {
    if (!needSlots || realBlocks.empty()) return;
    // one workgroup per span of a block's decoded bytes: a block is cut into equal spans of whole tiles, bins_span_tiles()
    // at the most (a block without records has nothing to count: its table stays zero)
    std::vector<D4GBinSpan> spans;
    const i64 maxTiles = bins_span_tiles();
    for (const int32_t bi : realBlocks) {
        const D4GBlock& b = hBlocks[bi];
        if (b.binStat < 0 || b.refCount == 0) continue;
        const i64 nTiles = (b.uLen + D4G_BINS_TILE - 1) / D4G_BINS_TILE, nSpans = (nTiles + maxTiles - 1) / maxTiles;
        const i64 per = (nTiles + nSpans - 1) / nSpans * D4G_BINS_TILE;
        for (i64 t0 = 0; t0 < b.uLen; t0 += per) spans.push_back({bi, (uint32_t)t0, (uint32_t)std::min<i64>(b.uLen, t0 + per)});
    }
    if (spans.empty()) return;
    D4GBinSpan* dSpans = tmp.upload(spans);
    D4GCtx c = make_ctx(engine().progDyn, 0);
    RT_LAUNCH(k_block_bins, spans.size(), bins_threads(), c, dSpans);
    stats.kernel_launches++;
}

}  // namespace d4g
