// Prints the launch plans (csrc/tn_multi_plan.h) of the problem lists that tests/test_tn_multi_plan_cpu.py pins: per launch
// its problems, their splits and modes, the grid and the placement table as one row per XCD.  Host only; built with the
// sanitizers it is the memory and undefined-behaviour check of the planner (not part of the test suite):
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -Iinclude -Iexploremultimodal_amd/csrc tools/tn_multi_plan_dump.cpp -o tn_multi_plan_dump && ./tn_multi_plan_dump
// Exit status 0: every list planned (or, for the two over-limit lists, was refused) as expected.
#include "tn_multi_plan.h"
#include <cstdio>

typedef std::vector<VlmoTnProblem> List;

static VlmoTnProblem prob(int M, int N1, int N2, int acc) { return VlmoTnProblem{nullptr, nullptr, nullptr, N1, N2, N2, M, N1, N2, 1.f, acc}; }

// the weight gradients of two transformer blocks: attention on M rows, one FFN per row count of `ffn`; longest first
static List blocks(int M, std::vector<int> ffn, int d, int hidden, int acc) {
    List l;
    for (int b = 0; b < 2; ++b) {
        l.push_back(prob(M, d, d, acc)), l.push_back(prob(M, 3 * d, d, acc));
        for (int m : ffn) l.push_back(prob(m, d, hidden, acc)), l.push_back(prob(m, hidden, d, acc));
    }
    std::stable_sort(l.begin(), l.end(), [](const VlmoTnProblem& a, const VlmoTnProblem& b) { return a.M > b.M; });
    return l;
}

static int dump(const char* name, const List& l, bool expect_error = false) {
    const TnMultiPlan plan = plan_tn_multi(l.data(), (int)l.size());
    printf("== %s: %zu problems\n", name, l.size());
    if (!plan.error.empty()) {
        printf("   error: %s\n", plan.error.c_str());
        return expect_error ? 0 : 1;
    }
    for (const TnLaunchPlan& L : plan.launches) {
        printf(" launch of problems [%d, %d): grid %d\n", L.q0, L.q0 + L.nq, L.grid);
        for (int q = 0; q < L.nq; ++q) {
            const VlmoTnProblem& r = l[L.q0 + q];
            const VlmoTnProblemPlan& s = L.p[q];
            printf("  %2d: M %5d N1 %5d N2 %5d  tiles %4d x %2d splits of %3d K-tiles  mode %d%s\n", q, r.M, r.N1, r.N2, s.tiles,
                   s.splits, s.kt_per_split, s.mode, s.zero_first ? "  zero first" : "");
        }
        for (int x = 0; x < 8; ++x) {
            printf("  xcd %d:", x);
            for (int b = x; b < L.grid; b += 8)
                L.order[b] == TN_NOP ? printf(" -") : printf(" %d.%d", L.order[b] >> 12, L.order[b] & 0xFFF);
            printf("\n");
        }
    }
    return expect_error ? 1 : 0;
}

int main() {
    int bad = 0;
    bad += dump("base, two experts, store", blocks(16704, {12608, 4096}, 768, 3072, 0));
    bad += dump("base, two experts, accumulate", blocks(16704, {12608, 4096}, 768, 3072, 1));
    bad += dump("base, fused", blocks(16704, {16704}, 768, 3072, 0));
    bad += dump("large, fused", blocks(8352, {8352}, 1024, 4096, 0));
    bad += dump("mini", blocks(22, {22}, 128, 512, 1));
    bad += dump("small", {prob(700, 256, 512, 1), prob(333, 96, 264, 0), prob(1000, 512, 256, 1)});
    bad += dump("split", {prob(2000, 256, 512, 1), prob(1333, 96, 264, 0), prob(3000, 512, 256, 1)});
    bad += dump("one base proj", {prob(16704, 768, 768, 0)});
    List many, wide;
    for (int i = 0; i < 19; ++i) many.push_back(prob(64 + 8 * i, 256, 264, 1));
    for (int i = 0; i < 20; ++i) wide.push_back(prob(64 * (1 + i % 3) + (i % 4 == 0 ? 5 : 0), 2048, 2048, i % 2 == 0));
    bad += dump("19 problems", many);
    bad += dump("20 x 64 tiles", wide);
    bad += dump("one problem of 1000 tiles", {prob(200, 6400, 10240, 0), prob(100, 256, 256, 1)});
    bad += dump("1056 tiles", {prob(64, 256 * 33, 256 * 32, 0)}, true);
    bad += dump("4160 tiles", {prob(64, 256 * 65, 256 * 64, 0)}, true);
    bad += dump("largest sizes", {prob(0x7FFFFFFF, 0x7FFFFFF8, 0x7FFFFFF8, 0)}, true);
    return bad;
}
