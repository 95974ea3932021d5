// d4g_host_search.h — Batch, candidate search: the executors' launchers and DeflateStream.optimise's per-block part.
#pragma once

namespace d4g {

// What only the level executor uses (candidate keys, the three memo tables): made on its first use — a batch the fused
// executor handles alone never allocates or clears them.
inline void Batch::ensure_level_tables() {
    if (dKeys || !levelBlocks) return;
    Engine& E = engine();
    const size_t nb = levelBlocks;
    dKeys.alloc(nb * (size_t)E.maxOps);
    dHsMemo.alloc_zero(nb * (size_t)D4G_HSMEMO_SLOTS);
    dPassMemo.alloc_zero((size_t)levelPassMemoWords, 64);
    dRcMemo.alloc_zero(nb * (size_t)D4G_RCMEMO_SLOTS);
}

// what both fused launchers hand their kernel
inline D4FParams Batch::fused_params(int maxRounds, D4GRoundResult* results, int32_t* info) {
    Engine& E = engine();
    D4FParams P;
    memset(&P, 0, sizeof(P));
    P.ops[0] = E.progDyn.dOps; P.ops[1] = E.progFixed.dOps;
    P.nOps[0] = (int)E.progDyn.ops.size(); P.nOps[1] = (int)E.progFixed.ops.size();
    P.maxRounds = maxRounds;
    P.regWords = fused_reg_words();
    P.caps = D4F_CAPS(fused_cap_masks(), fused_cap_codes(), fused_cap_hdrs());
    P.results = results;
    P.roundInfo = info;
    P.stats = fused_stats() ? E.dOpStats.get() : nullptr;
    return P;
}
// one launch of state ops over these blocks, for the roofline figures
inline void Batch::count_state_launch(const int32_t* blk, size_t n) {
    stats.state_launches++;
    for (size_t i = 0; i < n; i++) { stats.state_tokens_per_round += hBlocks[blk[i]].tokCount; stats.state_bytes_per_round += hBlocks[blk[i]].uLen; }
}

// the elements of v at the positions pos
template <typename T>
static std::vector<T> picked(const std::vector<T>& v, const std::vector<size_t>& pos) {
    std::vector<T> out;
    out.reserve(pos.size());
    for (size_t p : pos) out.push_back(v[p]);
    return out;
}
// The positions of `act` whose blocks the fused executor takes, one workgroup each, and the others.  Blocks of up to 16384
// back-references always; longer ones when there are many of them, which still fill the device one workgroup each (a few
// long blocks are left to an executor that gives each the whole device).
inline std::pair<std::vector<size_t>, std::vector<size_t>> Batch::split_for_fused(const std::vector<int>& act) const {
    std::pair<std::vector<size_t>, std::vector<size_t>> pos;
    size_t nLong = 0;
    for (int k : act) nLong += hBlocks[k].refCount > (1LL << 14);
    for (size_t i = 0; i < act.size(); i++) (hBlocks[act[i]].refCount <= fused_max_refs(nLong) ? pos.first : pos.second).push_back(i);
    return pos;
}

// One optimiseBlock call per block of `act`: the fused and cluster executors take the blocks they can hold, the level
// executor the rest.
inline std::vector<D4GRoundResult> Batch::run_round(const std::vector<int>& act) {
    if (!exec_fused()) return run_round_levels(act);
    std::vector<D4GRoundResult> res(act.size());
    auto [smallPos, bigPos] = split_for_fused(act);
    std::vector<int> small = picked(act, smallPos), big = picked(act, bigPos);
    if (!small.empty()) {
        std::vector<std::vector<D4GRoundResult>> ch = run_fused(small, 1);
        for (size_t i = 0; i < small.size(); i++) res[smallPos[i]] = ch[i].at(0);
    }
    if (!big.empty() && cluster_enabled()) {   // long merged blocks, one launch of the whole device each
        std::vector<int> rest;
        std::vector<size_t> restPos;
        for (size_t i = 0; i < big.size(); i++) {
            const D4GBlock& d = hBlocks[big[i]];
            D4GRoundResult r;
            if (d.refCount > cluster_min_refs() && (d.maskBase & 15) == 0 && (d.maskWords & 15) == 0 && (d.binMask & 15) == 0 && run_cluster(big[i], &r)) res[bigPos[i]] = r;
            else { rest.push_back(big[i]); restPos.push_back(bigPos[i]); }
        }
        big.swap(rest);
        bigPos.swap(restPos);
    }
    if (!big.empty()) {
        std::vector<D4GRoundResult> r = run_round_levels(big);
        for (size_t i = 0; i < big.size(); i++) res[bigPos[i]] = r[i];
    } else {
        stats.rounds++;
    }
    return res;
}
// One optimiseBlock round of one long block with every workgroup of the device (k_search_cluster).  false: the round did
// not fit the kernel's tables — the block is untouched and the caller uses another executor.
inline bool Batch::run_cluster(int blk, D4GRoundResult* out) {
    Engine& E = engine();
    rt().cur = 0;
    if (!dClArena) dClArena.alloc(1);
    rt_memset(dClArena, 0, 128);   // the epoch counter; every command slot is cleared by the control workgroup before use
    int32_t one = blk;
    rt_h2d(dActive, &one, sizeof(one));
    RtScratch tmp;
    D4GRoundResult* dRes = tmp.alloc<D4GRoundResult>(D4F_MAXROUNDS);
    int32_t* dInfo = tmp.alloc<int32_t>(4);
    D4GCtx c = make_ctx(E.progDyn, 1);
    const D4FParams P = fused_params(1, dRes, dInfo);
#ifdef D4G_HOSTSIM
    const int threads = fused_block();
#else
    const int threads = 512;
#endif
    RtEvent e0, e1;
    e0.record();
    RT_LAUNCH(k_search_cluster, cluster_wgs(), threads, c, P, dClArena, 0);
    e1.record();
    stats.kernel_launches++;
    count_state_launch(&one, 1);
    int32_t info = 0;
    rt_d2h(&info, dInfo, sizeof(info));
    D4GRoundResult r;
    rt_d2h(&r, dRes, sizeof(r));
    const float ms = rt_elapsed_ms(e0, e1);
    msSearch += ms;
    stats.ms_state_kernels += ms;
    tmp.release();
    if (debug_rounds()) fprintf(stderr, "cluster search: block of %lld back-references, %.3f ms%s\n", (long long)hBlocks[blk].refCount, ms, (info & D4F_INFO_FALLBACK) ? " (did not fit)" : "");
    if ((info & D4F_INFO_FALLBACK) || (info & 0xffff) < 1) { stats.cluster_fallbacks++; return false; }
    gpuType[blk] = r.newType;
    stats.rounds_fused += 1;
    stats.rounds_cluster += 1;
    *out = r;
    return true;
}
// Fused executor (k_search_fused): every block of `act` runs up to maxRounds optimiseBlock rounds, while it keeps
// improving, inside one workgroup.  Returns each block's chain of round results.  A round that does not fit the
// kernel's tables comes back untouched and is run by the level executor; the block then goes on here.
inline std::vector<std::vector<D4GRoundResult>> Batch::run_fused(const std::vector<int>& act, int maxRounds) {
    Engine& E = engine();
    std::vector<std::vector<D4GRoundResult>> chains(act.size());
    std::vector<int> todo(act.size());
    for (size_t i = 0; i < act.size(); i++) todo[i] = (int)i;
    RtScratch tmp;   // (run_round_levels below waits before it returns or throws its own errors)
    D4GRoundResult* dRes = nullptr;
    int32_t* dInfo = nullptr;
    while (!todo.empty()) {
        const int nA = (int)todo.size();
        std::vector<int32_t> sub(nA);
        for (int i = 0; i < nA; i++) sub[i] = act[todo[i]];
        rt().cur = 0;
        rt_h2d(dActive, sub.data(), sub.size() * sizeof(int32_t));
        if (!dRes) {
            dRes = tmp.alloc<D4GRoundResult>(act.size() * (size_t)D4F_MAXROUNDS);
            dInfo = tmp.alloc<int32_t>(act.size(), 16);
        }
        D4GCtx c = make_ctx(E.progDyn, nA);
        int cap = 0;   // most rounds any of them may still run
        for (int i = 0; i < nA; i++) cap = std::max(cap, maxRounds - (int)chains[todo[i]].size());
        const D4FParams P = fused_params(std::min(cap, fused_cap_rounds()), dRes, dInfo);
        RtEvent e0, e1;
        e0.record();
        RT_LAUNCH(k_search_fused, nA, fused_block(), c, P);
        e1.record();
        stats.kernel_launches++;
        count_state_launch(sub.data(), sub.size());
        std::vector<int32_t> info(nA);
        rt_d2h(info.data(), dInfo, (size_t)nA * sizeof(int32_t));
        std::vector<D4GRoundResult> r((size_t)nA * D4F_MAXROUNDS);
        rt_d2h(r.data(), dRes, r.size() * sizeof(D4GRoundResult));
        const float ms = rt_elapsed_ms(e0, e1);
        msSearch += ms;
        stats.ms_state_kernels += ms;
        if (debug_rounds()) fprintf(stderr, "fused search: %d blocks, up to %d rounds, %.3f ms\n", nA, P.maxRounds, ms);
        std::vector<int> next, fb;
        for (int i = 0; i < nA; i++) {
            const int n = info[i] & 0xffff;
            std::vector<D4GRoundResult>& ch = chains[todo[i]];
            for (int k = 0; k < n; k++) ch.push_back(r[(size_t)i * D4F_MAXROUNDS + k]);
            if (n) gpuType[sub[i]] = ch.back().newType;
            stats.rounds_fused += n;
            if (info[i] & D4F_INFO_FALLBACK) { fb.push_back(todo[i]); stats.fused_fallbacks_mid += n > 0; }
            else if ((info[i] & D4F_INFO_MORE) && (int)ch.size() < maxRounds) next.push_back(todo[i]);
        }
        if (!fb.empty()) {   // one round with the level executor, then back here if it improved
            std::vector<int> fbAct(fb.size());
            for (size_t i = 0; i < fb.size(); i++) fbAct[i] = act[fb[i]];
            std::vector<D4GRoundResult> rr = run_round_levels(fbAct);
            stats.fused_fallbacks += (int64_t)fb.size();
            for (size_t i = 0; i < fb.size(); i++) {
                chains[fb[i]].push_back(rr[i]);
                if (rr[i].improved && (int)chains[fb[i]].size() < maxRounds) next.push_back(fb[i]);
            }
        }
        std::sort(next.begin(), next.end());
        stats.fused_relaunches += (int64_t)next.size();
        todo.swap(next);
    }
    tmp.release();
    return chains;
}
// One pass (one program) of a level-executor round over `sub`, whose results go to res[subPos[k]]: one launch per program
// level, then the selection.  The active blocks are split into groups, one stream lane each: the launch tail of one group's
// level (a few long recode/tree ops) overlaps the other groups' levels.
inline void Batch::run_levels_pass(const Program& P, const std::vector<int32_t>& sub, const std::vector<size_t>& subPos, int pass, std::vector<D4GRoundResult>& res) {
    rt().cur = 0;
    const int nA = (int)sub.size();
    rt_h2d(dActive, sub.data(), sub.size() * sizeof(int32_t));
    RtEvent e0, e1, uploaded;
    uploaded.record();
    Events evs, keep, laneDone;
    e0.record();
    const int G = std::min(lanes(), std::max(1, nA / 16));
    for (int g = 0; g < G; g++) {
        int lo = (int)((i64)nA * g / G), hi = (int)((i64)nA * (g + 1) / G);
        if (hi <= lo) continue;
        rt().cur = g;
        D4GCtx c = make_ctx(P, hi - lo);
        c.active = dActive + lo;
        rt_stream_wait(uploaded);
        const i64 groups = (hi - lo + 7) / 8;   // d4g_map_wg
        // Level l's header searches read bases produced at level l-1, so they run on the lane's second
        // stream beside level l's state ops (the searches are LDS-bound at low occupancy).
        RtEvent* lvlPrev = nullptr;
        rt_stream2_wait(uploaded);
        for (int l = 0; l < P.nLevels; l++) {
            if (P.hdrOff[l].second) {
                if (lvlPrev) rt_stream2_wait(*lvlPrev);
                i64 grid = 8 * groups * P.hdrOff[l].second;
                RT_LAUNCH2(k_exec_hdr_search, grid, 64, c, P.dLists + P.hdrOff[l].first, P.hdrOff[l].second);
                stats.kernel_launches++;
            }
            if (P.stateOff[l].second) {
                i64 grid = 8 * groups * P.stateOff[l].second;
                evs.emplace_back(new RtEvent());
                evs.back()->record();
                RT_LAUNCH(k_exec_state_ops, grid, state_block(), c, P.dLists + P.stateOff[l].first, P.stateOff[l].second);
                evs.emplace_back(new RtEvent());
                evs.back()->record();
                stats.kernel_launches++;
                count_state_launch(sub.data() + lo, (size_t)(hi - lo));
            }
            keep.emplace_back(new RtEvent());
            keep.back()->record();
            lvlPrev = keep.back().get();
        }
        keep.emplace_back(new RtEvent());
        keep.back()->record2();
        rt_stream_wait(*keep.back());
        RT_LAUNCH(k_select, hi - lo, state_block(), c, dResults + lo);
        stats.kernel_launches++;
        laneDone.emplace_back(new RtEvent());
        laneDone.back()->record();
        stats.search_lanes = std::max<int64_t>(stats.search_lanes, G);   // most lanes any round of the batch used
    }
    rt().cur = 0;
    for (auto& ev : laneDone) rt_stream_wait(*ev);
    e1.record();
    std::vector<D4GRoundResult> r(sub.size());
    rt_d2h(r.data(), dResults, sub.size() * sizeof(D4GRoundResult));
    const float roundMs = rt_elapsed_ms(e0, e1);
    msSearch += roundMs;
    if (debug_rounds())
        fprintf(stderr, "search round %lld (%s program, levels): %d active blocks, %.3f ms\n", (long long)stats.rounds, pass == 0 ? "dynamic" : "fixed", nA, roundMs);
    for (size_t k = 0; k + 1 < evs.size(); k += 2) stats.ms_state_kernels += rt_elapsed_ms(*evs[k], *evs[k + 1]);
    for (size_t k = 0; k < sub.size(); k++) {
        res[subPos[k]] = r[k];
        gpuType[sub[k]] = r[k].newType;
    }
}
// One optimiseBlock call on every block of `act` with the level executor: the dynamic program over the blocks that are
// dynamic now, then the fixed one over the fixed ones.
inline std::vector<D4GRoundResult> Batch::run_round_levels(const std::vector<int>& act) {
    Engine& E = engine();
    ensure_level_tables();
    std::vector<D4GRoundResult> res(act.size());
    for (int pass = 0; pass < 2; pass++) {
        const Program& P = pass == 0 ? E.progDyn : E.progFixed;
        const int wantType = pass == 0 ? D4G_DYNAMIC : D4G_FIXED;
        std::vector<int32_t> sub;
        std::vector<size_t> subPos;
        for (size_t i = 0; i < act.size(); i++)
            if (gpuType[act[i]] == wantType) { sub.push_back(act[i]); subPos.push_back(i); }
        if (!sub.empty()) run_levels_pass(P, sub, subPos, pass, res);
    }
    stats.rounds++;
    return res;
}

// Winner of optimiseBlock given the device result and the stream position (stored candidate
// = DeflateStream.java:376-383, ranked right after op 0 "optimised").  Returns true when the
// stored candidate wins.
inline bool Batch::stored_wins(const D4GRoundResult& r, i64 uLen, i64 pos, i64* storedSize) {
    if (uLen > 65535) return false;
    i64 c = pos % 8;
    c = c == 0 ? 0 : 8 - c;
    i64 ss = (uLen + 4) * 8 + c;
    *storedSize = ss;
    if (ss < r.bestSize) return true;
    if (ss == r.bestSize && r.improved && r.bestSeq > 0) return true;
    return false;
}

// ---- DeflateStream.optimise, per-block part — DeflateStream.java:496-566 ----
inline void Batch::phase1() {
    // blocks the reference's loop reaches: it stops right after removing the first empty block
    std::vector<int> act;
    std::vector<std::pair<int, int>> owner;  // (stream, block index in stream)
    for (size_t si = 0; si < streams.size(); si++) {
        HStream& s = streams[si];
        if (s.status != 0) continue;
        for (size_t k = 0; k < s.blocks.size(); k++) {
            HBlock& b = s.blocks[k];
            bool sole = (k == 0 && s.blocks.size() == 1);
            if (b.uLen == 0 && !sole) break;
            if (b.type != D4G_STORED) { act.push_back(b.gpu); owner.push_back({(int)si, (int)k}); }
        }
    }
    if (exec_fused()) {   // all rounds of a block inside one workgroup; blocks the fused executor does not take follow below
        const auto [fusedPos, restPos] = split_for_fused(act);
        if (!fusedPos.empty()) {
            std::vector<std::vector<D4GRoundResult>> ch = run_fused(picked(act, fusedPos), 1 << 20);
            for (size_t i = 0; i < fusedPos.size(); i++) streams[owner[fusedPos[i]].first].blocks[owner[fusedPos[i]].second].chain = ch[i];
            stats.rounds++;
        }
        act = picked(act, restPos);
        owner = picked(owner, restPos);
    }
    // fixpoint rounds: every block follows its own chain of strictly improving Huffman states
    while (!act.empty()) {
        std::vector<D4GRoundResult> res = run_round_levels(act);
        std::vector<int> nact;
        std::vector<std::pair<int, int>> nowner;
        for (size_t i = 0; i < act.size(); i++) {
            HBlock& b = streams[owner[i].first].blocks[owner[i].second];
            b.chain.push_back(res[i]);
            if (res[i].improved) { nact.push_back(act[i]); nowner.push_back(owner[i]); }
        }
        act.swap(nact);
        owner.swap(nowner);
    }
    check_device_errors();
    // sequential resolution with the stream bit position (pos drift included)
    for (HStream& s : streams) {
        if (s.status != 0) continue;
        i64 pos = 0, saved = 0;
        bool first = true;
        size_t idx = 0;
        while (idx < s.blocks.size()) {
            bool finishPass = true;
            HBlock& b = s.blocks[idx];
            bool hasNext = idx + 1 < s.blocks.size();
            if (b.uLen > 0 || (first && !hasNext)) {
                pos += 3;
                if (b.type != D4G_STORED) {
                    size_t step = 0;
                    // chain index = number of improvements already applied to this block
                    while (step < b.chain.size() && b.chain[step].curSize != b.size) step++;
                    if (step >= b.chain.size()) throw std::runtime_error("phase1: chain lookup failed");
                    const D4GRoundResult& r = b.chain[step];
                    i64 ss = 0;
                    if (stored_wins(r, b.uLen, pos, &ss)) {
                        i64 cs = b.size - ss;
                        if (cs > 0) { saved += cs; b.type = D4G_STORED; finishPass = false; }
                    } else if (r.improved) {
                        saved += b.size - r.bestSize;
                        b.size = r.bestSize;
                        finishPass = false;
                    }
                }
                pos += b.size_at(pos);
            } else {
                saved += b.size_at(pos + 3) + 3;
                s.blocks.erase(s.blocks.begin() + idx);
                break;
            }
            if (finishPass) { idx++; first = false; }
        }
        s.saved = saved;
        // final Huffman type per block comes from the last round that ran on it
        for (HBlock& b : s.blocks)
            if (b.type != D4G_STORED) b.type = gpuType[b.gpu];
    }
}

}  // namespace d4g
