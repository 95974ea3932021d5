// d4g_host_merge.h — Batch, DeflateStream.mergeBlocks for all streams in lockstep.
#pragma once

namespace d4g {

// ---- DeflateStream.mergeBlocks — DeflateStream.java:568-650, all streams in lockstep ----
inline bool Batch::can_merge(const HBlock& a, const HBlock& b) {
    if (a.type == D4G_STORED) return a.uLen + b.uLen <= 65535;
    return b.type == D4G_FIXED || b.type == D4G_DYNAMIC;
}
// advance a stream's loop until it needs a device evaluation (returns true) or finishes
inline bool Batch::merge_advance(int si, MergeReq* req) {
    HStream& s = streams[si];
    while (s.mIdx < s.blocks.size()) {
        HBlock& cur = s.blocks[s.mIdx];
        bool hasNext = s.mIdx + 1 < s.blocks.size();
        bool finishPass = true;
        if (s.mFirst && !hasNext) {
            s.mPos += cur.size_at(s.mPos + 3) + 3;
        } else if (cur.uLen > 0) {
            s.mPos += 3;
            if (hasNext && can_merge(cur, s.blocks[s.mIdx + 1])) {
                HBlock& next = s.blocks[s.mIdx + 1];
                if (cur.type == D4G_STORED) {  // DeflateBlockUncompressed.merge — :112-117 (host only)
                    HBlock m = cur;
                    m.uLen = cur.uLen + next.uLen;
                    m.tokCount = 0;
                    i64 curNo = cur.size_at(s.mPos);
                    i64 nextNo = next.size_at(s.mPos + curNo + 3);
                    i64 cs = (curNo + 3 + nextNo) - m.size_at(s.mPos);
                    if (cs > 0) {
                        s.mSaved += cs;
                        s.blocks[s.mIdx] = m;
                        s.blocks.erase(s.blocks.begin() + s.mIdx + 1);
                        finishPass = false;
                    }
                } else {
                    int ar = cur.gpu == s.arena[0] ? s.arena[1] : s.arena[0];
                    D4GBlock& d = hBlocks[ar];
                    d.tokStart = cur.tokStart;
                    d.tokCount = cur.tokCount + next.tokCount;
                    d.refStart = cur.refStart;
                    d.refCount = cur.refCount + next.refCount;
                    d.uStart = cur.uStart;
                    d.uLen = cur.uLen + next.uLen;
                    d.maskWords = (d.refCount + 63) / 64;
                    if (d.refCount > cluster_min_refs()) d.maskWords = (d.maskWords + 15) & ~15LL;   // whole 128-byte lines (zero padding): see layout_blocks
                    d.type = D4G_FIXED;
                    req->stream = si;
                    req->arena = ar;
                    s.mWaiting = true;
                    return true;
                }
            }
            s.mPos += s.blocks[s.mIdx].size_at(s.mPos);
        } else {
            s.mSaved += cur.size_at(s.mPos + 3) + 3;
            s.blocks.erase(s.blocks.begin() + s.mIdx);
            break;
        }
        if (finishPass) { commit_block(si, s.mIdx); s.mIdx++; s.mFirst = false; }
    }
    s.mDone = true;
    return false;
}
inline void Batch::merge_apply(int si, int arena, const D4GRoundResult& r) {
    HStream& s = streams[si];
    HBlock& cur = s.blocks[s.mIdx];
    HBlock& next = s.blocks[s.mIdx + 1];
    i64 uLen = cur.uLen + next.uLen;
    i64 curNo = cur.size_at(s.mPos);
    i64 nextNo = next.size_at(s.mPos + curNo + 3);
    HBlock m;
    m.tokStart = cur.tokStart;
    m.tokCount = cur.tokCount + next.tokCount;
    m.refStart = cur.refStart;
    m.refCount = cur.refCount + next.refCount;
    m.homeGpu = cur.homeGpu;
    m.ordinal = cur.ordinal;
    m.uStart = cur.uStart;
    m.uLen = uLen;
    i64 ss = 0;
    if (stored_wins(r, uLen, s.mPos, &ss)) { m.type = D4G_STORED; m.gpu = -1; m.size = 0; }
    else { m.type = r.newType; m.gpu = arena; m.size = r.bestSize; }
    i64 cs = (curNo + 3 + nextNo) - m.size_at(s.mPos);
    bool finishPass = true;
    if (cs > 0) {
        s.mSaved += cs;
        s.blocks[s.mIdx] = m;
        s.blocks.erase(s.blocks.begin() + s.mIdx + 1);
        finishPass = false;
    }
    s.mPos += s.blocks[s.mIdx].size_at(s.mPos);
    if (finishPass) { commit_block(si, s.mIdx); s.mIdx++; s.mFirst = false; }
    s.mWaiting = false;
}
// A merged block that the walk has finished with lives in one of the stream's two arenas, which the next chain of
// merges will overwrite: move its descriptor, state and mask to the device block of the first parsed block it covers
// (that block is dead now) and to the stream's commit mask area (disjoint by construction: word offset =
// first record / 64 + position of that first block).
inline void Batch::commit_block(int si, size_t idx) {
    HStream& s = streams[si];
    HBlock& hb = s.blocks[idx];
    if (hb.gpu < 0 || (hb.gpu != s.arena[0] && hb.gpu != s.arena[1])) return;
    const int home = hb.homeGpu;
    D4GBlock d = hBlocks[hb.gpu];
    d.stateIdx = hBlocks[home].stateIdx;
    d.maskBase = s.commitMaskBase + ((hb.refStart - s.refBase) >> 6) + hb.ordinal;
    d.maskWords = (hb.refCount + 63) / 64;
    d.binStat = -1;
    d.passMemo = -1;
    hBlocks[home] = d;
    gpuType[home] = gpuType[hb.gpu];
    patch_block(home);
    pendingCommits.push_back({hb.gpu, 0, home, 0});
    hb.gpu = home;
}
// descriptor changes are collected and applied by one upload + one scatter kernel (k_patch_blocks)
inline void Batch::patch_block(int idx) { blockPatches[idx] = hBlocks[idx]; }
inline void Batch::flush_block_patches() {
    if (blockPatches.empty()) return;
    std::vector<int32_t> idx;
    std::vector<D4GBlock> src;
    for (auto& kv : blockPatches) { idx.push_back(kv.first); src.push_back(kv.second); }
    blockPatches.clear();
    RtScratch tmp;
    int32_t* dIdx = tmp.alloc<int32_t>(idx.size());
    D4GBlock* dSrcB = tmp.alloc<D4GBlock>(src.size());
    rt_h2d(dIdx, idx.data(), idx.size() * 4);
    rt_h2d(dSrcB, src.data(), src.size() * sizeof(D4GBlock));
    RT_LAUNCH(k_patch_blocks, idx.size(), 64, dBlocks, dIdx, dSrcB, (int)idx.size());
    stats.kernel_launches++;
    rt_sync();   // (the staging buffers go back to the pool)
    tmp.release();
}
inline void Batch::flush_commits(D4GMergeJob* dJobs) {
    flush_block_patches();
    if (pendingCommits.empty()) return;
    rt_h2d(dJobs, pendingCommits.data(), pendingCommits.size() * sizeof(D4GMergeJob));
    D4GCtx c = make_ctx(engine().progFixed, 0);
    RT_LAUNCH(k_commit_merged, pendingCommits.size(), 256, c, dJobs);
    stats.kernel_launches++;
    rt_sync();   // (the job list is re-used right away)
    pendingCommits.clear();
}
inline void Batch::phase_merge() {
    Engine& E = engine();
    RtScratch tmp;
    D4GMergeJob* dJobs = tmp.alloc<D4GMergeJob>(2 * streams.size(), 64);
    while (true) {
        std::vector<MergeReq> reqs;
        std::vector<D4GMergeJob> jobs;
        for (size_t si = 0; si < streams.size(); si++) {
            HStream& s = streams[si];
            if (s.status != 0 || s.mDone) continue;
            MergeReq rq;
            if (merge_advance((int)si, &rq)) {
                reqs.push_back(rq);
                D4GMergeJob j;
                j.blkA = s.blocks[s.mIdx].gpu;
                j.blkB = s.blocks[s.mIdx + 1].gpu;
                j.blkM = rq.arena;
                j.pad = 0;
                jobs.push_back(j);
                patch_block(rq.arena);
            }
        }
        flush_commits(dJobs);   // before any arena is overwritten
        if (reqs.empty()) break;
        rt_h2d(dJobs, jobs.data(), jobs.size() * sizeof(D4GMergeJob));
        D4GCtx c = make_ctx(E.progFixed, 0);
        RT_LAUNCH(k_make_merged, jobs.size(), state_block(), c, dJobs);
        stats.kernel_launches++;
        std::vector<int> act;
        for (auto& rq : reqs) { act.push_back(rq.arena); gpuType[rq.arena] = D4G_FIXED; }
        std::vector<D4GRoundResult> res = run_round(act);
        for (size_t i = 0; i < reqs.size(); i++) merge_apply(reqs[i].stream, reqs[i].arena, res[i]);
    }
    tmp.release();   // (every round above ended in a wait)
    flush_block_patches();
    check_device_errors();
    for (HStream& s : streams)
        if (s.status == 0) s.saved += s.mSaved;
}

}  // namespace d4g
