// gemm_nt, 32x32x16 MFMA (gemm_nt_kernel, gemm_common.h), and the front end of every NT GEMM: argument checks, the tile
// planner that picks between these kernels and the 16x16x32 ones of gemm_nt16.hip, the grouped launch, and the registry
// of the GEMM profiling hooks.
#include "gemm_common.h"
#include <mutex>
#include <vector>

namespace vlmo_prof {
struct ProfRec {
    hipEvent_t a, b;
    int tag;
    double flops;
};
struct Prof {
    std::vector<ProfRec> recs;
    size_t used = 0;
    bool on = false;
    std::mutex mu;
} g_prof;

ProfScope::ProfScope(int tag, double flops, hipStream_t s) : st(s) {
    if (!g_prof.on) return;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    if (g_prof.used < g_prof.recs.size()) {
        r = &g_prof.recs[g_prof.used++];
        r->tag = tag;
        r->flops = flops;
        (void)hipEventRecord(r->a, st);
    }
}
ProfScope::~ProfScope() {
    if (r) (void)hipEventRecord(r->b, st);
}

extern "C" int vlmo_profile_start(int max_records) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    while ((int)g_prof.recs.size() < max_records) {
        ProfRec r{};
        if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) {
            vlmo_set_error("vlmo_profile_start: hipEventCreate failed");
            return -1;
        }
        g_prof.recs.push_back(r);
    }
    g_prof.used = 0;
    g_prof.on = true;
    return 0;
}

// Stops recording and sums per tag (tag = epilogue id for gemm_nt, +16 when the 256x256 tile ran; 32 + epilogue for
// conv; 48 + epilogue for the 256x128 tile; 64 / 72 for gemm_tn 128x128 / 256x256, 73 for gemm_tn_multi; 80 + epilogue for
// the 16x16x32 kernels of any tile height).  Call after the stream(s) have been synchronised.
extern "C" int vlmo_profile_stop(int ntags, double* ms, double* flops, int64_t* launches) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.on = false;
    for (int i = 0; i < ntags; ++i) {
        ms[i] = 0;
        flops[i] = 0;
        launches[i] = 0;
    }
    for (size_t i = 0; i < g_prof.used; ++i) {
        const ProfRec& r = g_prof.recs[i];
        float t = 0.f;
        if (r.tag < 0 || r.tag >= ntags || hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) continue;
        ms[r.tag] += t;
        flops[r.tag] += r.flops;
        launches[r.tag] += 1;
    }
    return (int)g_prof.used;
}
}  // namespace vlmo_prof

namespace {
int check_nt(int epi, const void* A, int lda, const void* B, int ldb, int M, int N, int K, const VlmoEpilogue* e) {
    VLMO_CHECK_ARG(A && B && e, "vlmo_gemm_nt: null operand");
    VLMO_CHECK_ARG(M > 0 && N > 0 && K > 0, "vlmo_gemm_nt: empty problem M=%d N=%d K=%d", M, N, K);
    VLMO_CHECK_ARG(K % 64 == 0, "vlmo_gemm_nt: K=%d must be a multiple of 64", K);
    VLMO_CHECK_ARG(N % 4 == 0, "vlmo_gemm_nt: N=%d must be a multiple of 4", N);
    VLMO_CHECK_ARG(lda % 8 == 0 && ldb % 8 == 0 && lda >= K && ldb >= K, "vlmo_gemm_nt: bad lda/ldb %d/%d", lda, ldb);
    VLMO_CHECK_ARG(e->out && (epi == VLMO_EPI_ARGMAX || epi == VLMO_EPI_CE || (e->ldo >= N && e->ldo % 4 == 0)), "vlmo_gemm_nt: bad output / ldo");
    VLMO_CHECK_ARG(epi != VLMO_EPI_CE || (e->ldo >= (N + 63) / 64 && e->row_index), "vlmo_gemm_nt: cross-entropy epilogue needs labels and ldo >= chunks");
    VLMO_CHECK_ARG(epi != VLMO_EPI_CE_BWD || (e->resid && e->row_scale && e->row_index), "vlmo_gemm_nt: cross-entropy backward needs lse, row scale, labels");
    VLMO_CHECK_ARG(epi != VLMO_EPI_BIAS_GELU || (e->out2 && e->ld2 >= N), "vlmo_gemm_nt: gelu epilogue needs out2");
    VLMO_CHECK_ARG(epi != VLMO_EPI_ARGMAX || e->ldo >= (N + 63) / 64, "vlmo_gemm_nt: argmax partial buffer too narrow");
    VLMO_CHECK_ARG(epi != VLMO_EPI_RESID || e->resid, "vlmo_gemm_nt: residual epilogue needs resid");
    VLMO_CHECK_ARG(epi != VLMO_EPI_DGELU || (e->aux && e->ld2 >= N), "vlmo_gemm_nt: dgelu epilogue needs aux");
    return 0;
}

int run_nt(int epi, int dtype, int tile, GemmNTGroups& gp, hipStream_t stream) {
    VLMO_CHECK_ARG(dtype == VLMO_BF16 || dtype == VLMO_F16, "vlmo_gemm_nt: dtype must be bf16 or f16");
    const int tile_in = tile;
    long Mtot = 0;
    for (int q = 0; q < gp.ngroups; ++q) Mtot += gp.g[q].M;
    const int N = gp.g[0].N, K = gp.g[0].K;
    if (tile < 0) {
        // measured on MI355X (tools/gemm_bench.py): deep reductions want the 256x256 ping-pong kernel (half
        // the staged bytes per flop, MFMA pipe and LDS port busy at the same time, one workgroup/CU);
        // shallow ones (K = d) are epilogue bound and want two 128x128 workgroups per CU so that one's
        // stores overlap the other's MFMAs
        tile = (K >= 1536 && Mtot >= 2048 && N >= 512) ? 3 : 0;
        // shallow reductions whose 256x256 tiles fit ONE dispatch round (proj, dgrad_proj at N = d: 198 tiles) also do
        // better with the big tile: 1 round instead of 1.53 -> 2 rounds of 128x128 (42 vs 47 us, 30 vs 34 us)
        if (tile == 0 && K >= 512 && N >= 512 && Mtot >= 2048) {
            long t256 = 0;
            for (int q = 0; q < gp.ngroups; ++q) t256 += (long)((gp.g[q].M + 255) / 256) * ((N + 255) / 256);
            if (t256 <= 256) tile = 3;
        }
        // fewer than 128 tiles of 256x256 (the text-only pass of the four-loss objective: 2 048 rows) leave most CUs without
        // work whatever the reduction depth: 128x128 tiles, one or two per CU (tools/nt16_bench.py --M 2048, N = 768, K = 3 072:
        // 76 us with 24 tiles of 256x256, 62 with 192x256, 36.5 with 96 of 128x128)
        long t256_all = 0;
        for (int q = 0; q < gp.ngroups; ++q) t256_all += (long)((gp.g[q].M + 255) / 256) * ((N + 255) / 256);
        const bool few_tiles = t256_all <= 128;
        if (few_tiles) tile = 0;
        if (tile == 0 && dtype == VLMO_BF16 && (epi == VLMO_EPI_BIAS || epi == VLMO_EPI_BIAS_GELU) && K <= 1024 && N >= 2048 && Mtot >= 4096)
            tile = 4;
        // 192-row ping-pong tiles when they cut the dispatch rounds (VLMo-Large at 32 pairs: M = 8 352 = 32.6 x 256, so
        // N = 1 024 is 132 tiles of 256x256 on 256 CUs but 176 tiles of 192x256, each 3/4 of the work)
        if (!few_tiles && dtype == VLMO_BF16 && (epi == VLMO_EPI_BIAS || epi == VLMO_EPI_BIAS_GELU || epi == VLMO_EPI_RESID || epi == VLMO_EPI_DGELU) && K >= 1024) {
            long t256 = 0, t192n = 0;
            for (int q = 0; q < gp.ngroups; ++q) {
                t256 += (long)((gp.g[q].M + 255) / 256) * ((N + 255) / 256);
                t192n += (long)((gp.g[q].M + 191) / 192) * ((N + 255) / 256);
            }
            const long e256 = ((t256 + 255) / 256) * 256, e192 = ((t192n + 255) / 256) * 192;
            if (e192 * 10 <= e256 * 9) tile = 8;
        }
    }
    // 16x16x32 tiles of (16 * H16) x 256, H16 = 9 .. 20: the height is chosen so that the tiles fill whole dispatch rounds of
    // the 256 CUs.  Cost model (tools/nt16_bench.py at M = 2 048 ... 33 408, profiles/r04_nt16_*.txt): a launch costs
    // rounds x (H16 + 26), rounds = ceil(tiles / 256) -- a K-tile of a (16 H16) x 256 tile stages 16 (H16 + 16) rows through the
    // CU's fill path, and a tile-round carries a fixed part worth ~10 more (prologue, epilogue, launch): 144 against 192 rows
    // measured 0.92 - 0.94 x (model 0.92), 160 against 208 0.93 - 0.95 (0.92), three rounds of 272 against four of 256 0.87
    // (0.77).  The tiles picked above cost, in the same units: 256x256 rounds x 42, 192x256 rounds x 38, 256x128x32 (two per
    // CU, the epilogue of one under the K loop of the other) rounds-of-512 x 38, 128x128 rounds-of-512 x 21 (16 when every
    // tile has a CU to itself).
    // at EQUAL tile height the 16x16x32 kernel is 4 - 8 % faster than the 32x32x16 ones (DMA issued in the read segment;
    // tools/nt16_bench.py at M = 12 608 / 33 408, profiles/r04_nt16_bigM.txt), so a tie in the model goes to it; problems from
    // 40 output tiles of 256 x 256 up (M = 12 608 at N = 768: 42 -> 36 us).  In-session A/Bs of the full four-loss objective
    // (B = 32, merged passes): (97 %, 150 tiles) -> (102, 100) -1.0 ms, -> (106, 40) another -1.3 ms, (110, 16) no further
    // change; VLMo-Large -0.3 ms (its N = 1 024 GEMMs at 8 352 rows were below the old threshold), VLMo-Base unchanged.
    if ((tile == 0 || tile == 3 || tile == 4 || tile == 8) && dtype == VLMO_BF16 && !gp.g[0].k1 && !gp.g[0].ckw &&
        (epi == VLMO_EPI_BIAS || epi == VLMO_EPI_BIAS_GELU || epi == VLMO_EPI_RESID || epi == VLMO_EPI_DGELU) && N >= 512 && K >= 512 &&
        Mtot * (long)N >= 40 * 65536l && tile_in < 0) {
        auto count = [&](int bm, int bn) {
            long t = 0;
            for (int q = 0; q < gp.ngroups; ++q) t += (long)((gp.g[q].M + bm - 1) / bm) * ((N + bn - 1) / bn);
            return t;
        };
        double cur;
        if (tile == 3) cur = (double)((count(256, 256) + 255) / 256) * 42;
        else if (tile == 8) cur = (double)((count(192, 256) + 255) / 256) * 38;
        else if (tile == 4) cur = (double)((count(256, 128) + 511) / 512) * 38;
        else cur = count(128, 128) <= 256 ? 16.0 : (double)((count(128, 128) + 511) / 512) * 21;
        int best = 0;
        double bc = 1e30;
        for (int h16 = 9; h16 <= 20; ++h16) {
            const double c = (double)((count(16 * h16, 256) + 255) / 256) * (h16 + 26);
            if (c < bc) bc = c, best = h16;
        }
        if (bc * 100 <= cur * 106) tile = 300 + best;
    }
    if (tile >= 106 && tile <= 110) tile = 300 + 2 * (tile - 100);      // (32 * (tile - 100)) rows = an even H16
    if (tile >= 309 && tile <= 320) {
        // 16x16x32 MFMA, (16 * (tile - 300)) x 256 tile: bf16, plain GEMM (no convolution, no second segment)
        VLMO_CHECK_ARG(dtype == VLMO_BF16 && !gp.g[0].k1, "vlmo_gemm_nt: tiles 106..110 / 309..320 are bf16, single-source");
        ProfScope prof(80 + epi, 2.0 * Mtot * N * K, stream);
        return launch_nt16_height(tile - 300, epi, gp, stream);
    }
    VLMO_CHECK_ARG(tile == 0 || tile == 3 || tile == 4 || tile == 8, "vlmo_gemm_nt: tile must be -1, 0, 3, 4, 8, 106..110 or 309..320 (got %d)", tile);
    if (tile == 4 && !(dtype == VLMO_BF16 && (epi == VLMO_EPI_BIAS || epi == VLMO_EPI_BIAS_GELU))) tile = 0;
    if (tile == 8 && !(dtype == VLMO_BF16 && (epi == VLMO_EPI_BIAS || epi == VLMO_EPI_BIAS_GELU || epi == VLMO_EPI_RESID || epi == VLMO_EPI_DGELU))) tile = 3;
    ProfScope prof(epi + (tile == 3 || tile == 8 ? 16 : (tile == 4 ? 48 : 0)), 2.0 * Mtot * N * K, stream);
    // tile 4 = 256x128x32, four waves, two workgroups per CU (bf16; bias and bias+GELU epilogues only): the wide shallow
    // GEMMs (qkv, fc1: K = d, N >= 3d).  1.5x the staged bytes per flop of 256x256 instead of the 2x of 128x128, still two
    // desynchronised workgroups per CU, finer tile quantisation: fc1 119 -> 113 us, qkv 80 -> 75 us.
    if (tile == 4)
        return launch_nt<bf16, 256, 128, 2, 2, false, 32, 2, false, (1u << VLMO_EPI_BIAS) | (1u << VLMO_EPI_BIAS_GELU)>(epi, gp, stream);
    if (tile == 8)
        return launch_nt<bf16, 192, 256, 2, 4, false, 64, 2, true,
                         (1u << VLMO_EPI_BIAS) | (1u << VLMO_EPI_BIAS_GELU) | (1u << VLMO_EPI_RESID) | (1u << VLMO_EPI_DGELU)>(epi, gp, stream);
    if (dtype == VLMO_F16) {
        if (tile == 3) return launch_nt<f16, 256, 256, 2, 4, false, 64, 2, true>(epi, gp, stream);
        return launch_nt<f16, 128, 128, 2, 2>(epi, gp, stream);
    }
    if (tile == 3) return launch_nt<bf16, 256, 256, 2, 4, false, 64, 2, true>(epi, gp, stream);
    return launch_nt<bf16, 128, 128, 2, 2>(epi, gp, stream);
}

// Row-tiles per group of the L2 tile order, by the bytes of the weight matrix: a group is group_m row panels against ALL column tiles, so group_m = 1 streams the whole weight once per row
// panel -- cheap while the weight is of the size of an XCD's L2 (4 MB), and then the activation panel is fetched once;
// larger weights want their column tiles reused across several row panels.  In-step sweeps (tools/ab_multi.sh, weight
// gradients on the main stream): VLMo-Base (weights <= 4.7 MB) group_m 1 / 2 / 3 / 4 = 14.34 / 14.36 / 14.38 / 14.43 ms;
// VLMo-Large (2 - 8.4 MB) 24.88 against 24.79 at 4; the dVAE encoder (output convolution: 67 MB) 6.03 against 5.92 ms at 4.
// (Under the side stream round 3 had measured 2 - 6 equal, 8 +0.1 ms, 16 +0.35 ms.)
int group_m_for(int N, int K) {
    return (long)N * K * 2 <= 5l << 20 ? 1 : 4;
}
}  // namespace

extern "C" int vlmo_gemm_nt(int epi, int dtype, int tile, const void* A, int lda, const void* B, int ldb,
                            int M, int N, int K, const VlmoEpilogue* e, hipStream_t stream) {
    if (int rc = check_nt(epi, A, lda, B, ldb, M, N, K, e)) return rc;
    GemmNTGroups gp{};
    gp.ngroups = 1;
    gp.g[0] = GemmNT{A, B, M, N, K, lda, ldb, *e, 0, 0, 0, 0, nullptr, group_m_for(N, K), nullptr, 0, 0, 1.f};
    return run_nt(epi, dtype, tile, gp, stream);
}

extern "C" int vlmo_gemm_nt_2src(int epi, int dtype, int tile, const void* A, int lda, int k1, float seg_scale,
                                 const void* A2, int lda2, const void* B, int ldb, int M, int N, int K,
                                 const VlmoEpilogue* e, hipStream_t stream) {
    VLMO_CHECK_ARG(A2 && k1 > 0 && k1 < K && k1 % 64 == 0, "vlmo_gemm_nt_2src: need 0 < k1 < K, k1 %% 64 == 0 (k1=%d, K=%d)", k1, K);
    VLMO_CHECK_ARG(dtype == VLMO_F16, "vlmo_gemm_nt_2src: instantiated for f16 (the dVAE encoder) only");
    VLMO_CHECK_ARG(lda % 8 == 0 && lda >= k1 && lda2 % 8 == 0 && lda2 >= K - k1, "vlmo_gemm_nt_2src: bad lda/lda2 %d/%d", lda, lda2);
    if (int rc = check_nt(epi, A, K > lda ? K : lda, B, ldb, M, N, K, e)) return rc;
    GemmNTGroups gp{};
    gp.ngroups = 1;
    gp.g[0] = GemmNT{A, B, M, N, K, lda, ldb, *e, 0, 0, 0, 0, nullptr, group_m_for(N, K), A2, lda2, k1, seg_scale};
    return run_nt(epi, dtype, tile, gp, stream);
}

extern "C" int vlmo_gemm_nt_grouped(int epi, int dtype, int tile, int ngroups, const void* const* A, int lda,
                                    const void* const* B, int ldb, const int32_t* M, int N, int K,
                                    const VlmoEpilogue* e, hipStream_t stream) {
    VLMO_CHECK_ARG(ngroups >= 1 && ngroups <= MAX_GROUPS && A && B && M && e, "vlmo_gemm_nt_grouped: 1..%d groups", MAX_GROUPS);
    VLMO_CHECK_ARG(epi != VLMO_EPI_ARGMAX && epi != VLMO_EPI_CE, "vlmo_gemm_nt_grouped: the arg-max / cross-entropy epilogues are single-problem");
    GemmNTGroups gp{};
    gp.ngroups = ngroups;
    for (int q = 0; q < ngroups; ++q) {
        if (int rc = check_nt(epi, A[q], lda, B[q], ldb, M[q], N, K, &e[q])) return rc;
        gp.g[q] = GemmNT{A[q], B[q], M[q], N, K, lda, ldb, e[q], 0, 0, 0, 0, nullptr, group_m_for(N, K), nullptr, 0, 0, 1.f};
    }
    return run_nt(epi, dtype, tile, gp, stream);
}
