// The launch plan of vlmo_gemm_tn_multi: which problems share a launch, how each problem's token dimension is split,
// which epilogue it gets, which outputs are zeroed first and which workgroup of the grid runs which tile.  THE definition:
// the launcher executes what plan_tn_multi returns and vlmo_gemm_tn_multi_plan serialises it (tests/test_tn_multi_plan_cpu.py
// pins it without a GPU).  Host code only, no HIP runtime call; reads the shapes and the accumulate flag of a problem, never
// its pointers.
#pragma once
#include "vlmo_hip.h"
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

// One launch takes up to MAX_TN_PROBS problems of 256x256 tiles.  Workgroup b of it runs order[b] = (problem << 12) |
// (workgroup index inside the problem), or nothing (TN_NOP).  The table is filled so that the workgroups one XCD receives
// (b % 8 equal, dealt round-robin) are a BALANCED mix: with problems of different reduction lengths in one launch (below the
// fusion layer: 261, 197 and 64 K-tiles) contiguous XCD chunks gave one XCD 45 long tiles for its 32 CUs -- two rounds,
// 1 035 us instead of 525 -- while another finished its 45 short ones in a quarter of the time.
constexpr int MAX_TN_PROBS = 16;
constexpr int MAX_TN_ORDER = 1024;
constexpr uint16_t TN_NOP = 0xFFFF;
// epilogue of a tile: fp32 atomics into C (the token dimension is split over several workgroups), C += alpha * acc or
// C = alpha * acc (the workgroup owns the tile)
enum { TN_ATOMIC = 0, TN_ACCUM = 1, TN_STORE = 2 };

struct TnLaunchPlan {
    int q0, nq;                              // problems [q0, q0 + nq) of the call
    VlmoTnProblemPlan p[MAX_TN_PROBS];
    int grid;                                // workgroups = used entries of order
    uint16_t order[MAX_TN_ORDER];
};
struct TnMultiPlan {
    std::vector<TnLaunchPlan> launches;
    std::string error;                       // not empty: the call cannot be planned, launches is meaningless
};

// 256x256 output tiles and 64-token K-tiles of a problem (64-bit: no shape overflows them)
inline int64_t tn_tiles256(const VlmoTnProblem& r) { return (((int64_t)r.N1 + 255) / 256) * (((int64_t)r.N2 + 255) / 256); }
inline int tn_ktiles(const VlmoTnProblem& r) { return (int)(((int64_t)r.M + 63) / 64); }

inline TnMultiPlan plan_tn_multi(const VlmoTnProblem* probs, int n) {
    TnMultiPlan plan;
    char msg[128];
    auto fail = [&](const char* fmt, auto... a) {
        snprintf(msg, sizeof msg, fmt, a...);
        plan.error = msg;
        return plan;
    };
    for (int q = 0; q < n; ++q)
        if (probs[q].M < 1 || probs[q].N1 < 1 || probs[q].N2 < 1)
            return fail("vlmo_gemm_tn_multi: bad shape in problem %d (M=%d N1=%d N2=%d)", q, probs[q].M, probs[q].N1, probs[q].N2);
    for (int q0 = 0, nq = 0; q0 < n; q0 += nq) {
        // one launch = as many of the remaining problems as fit the problem table and the placement table
        int64_t tiles_all = 0;
        for (nq = 0; q0 + nq < n && nq < MAX_TN_PROBS; ++nq) {
            const int64_t t = tn_tiles256(probs[q0 + nq]);
            if (nq > 0 && tiles_all + t > MAX_TN_ORDER - 64) break;
            tiles_all += t;
        }
        // fewer than ~3/4 of the CUs' worth of tiles: split every problem's token dimension, but leave a workgroup at
        // least 8 K-tiles of the shortest reduction
        int min_nk = 1 << 30;
        for (int q = 0; q < nq; ++q) min_nk = std::min(min_nk, tn_ktiles(probs[q0 + q]));
        const int splits = tiles_all >= 192 ? 1 : std::max(1, std::min((int)(256 / tiles_all), min_nk / 8));
        plan.launches.emplace_back();
        TnLaunchPlan& L = plan.launches.back();
        L.q0 = q0, L.nq = nq;
        struct Job {
            uint16_t code;
            int cost;
        };
        std::vector<Job> jobs;
        for (int q = 0; q < nq; ++q) {
            const VlmoTnProblem& r = probs[q0 + q];
            const int64_t tiles = tn_tiles256(r);
            const int nk = tn_ktiles(r);
            int sp = std::min(splits, nk);
            const int per = (nk + sp - 1) / sp;
            sp = (nk + per - 1) / per;
            if (tiles * sp > 4096) return fail("vlmo_gemm_tn_multi: problem %d has too many tiles", q0 + q);
            const int mode = sp > 1 ? TN_ATOMIC : r.accumulate ? TN_ACCUM : TN_STORE;
            L.p[q] = VlmoTnProblemPlan{(int)tiles, sp, per, mode, sp > 1 && !r.accumulate};
            for (int l = 0; l < (int)tiles * sp; ++l) jobs.push_back(Job{(uint16_t)((q << 12) | l), per});
        }
        // placement: classes of equal reduction length, longest first; every class is cut into 8 contiguous runs (a
        // run = neighbouring tiles of one problem: they share operand panels through the XCD's L2) and XCD x takes run
        // x of every class, so all XCDs get the same mix and, inside an XCD, long tiles are dispatched before short ones
        std::stable_sort(jobs.begin(), jobs.end(), [](const Job& a, const Job& b) { return a.cost > b.cost; });
        std::vector<uint16_t> bins[8];
        for (size_t i = 0, j; i < jobs.size(); i = j) {
            for (j = i; j < jobs.size() && jobs[j].cost == jobs[i].cost;) ++j;
            const size_t cnt = j - i;
            for (int x = 0; x < 8; ++x)
                for (size_t k = i + cnt * x / 8; k < i + cnt * (x + 1) / 8; ++k) bins[x].push_back(jobs[k].code);
        }
        size_t deepest = 0;
        for (int x = 0; x < 8; ++x) deepest = std::max(deepest, bins[x].size());
        if (deepest * 8 > (size_t)MAX_TN_ORDER)
            return fail("vlmo_gemm_tn_multi: %zu workgroups exceed one launch (pass fewer problems per call)", jobs.size());
        L.grid = (int)deepest * 8;
        for (int b = 0; b < L.grid; ++b) {
            const std::vector<uint16_t>& bin = bins[b & 7];
            L.order[b] = (size_t)(b >> 3) < bin.size() ? bin[b >> 3] : TN_NOP;
        }
    }
    return plan;
}
