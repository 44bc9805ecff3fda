// The VLMo Blocks (vlmo.py:187-197) of one backbone pass forward / backward per C-ABI call: native
// orchestration of the kernels in gemm_*.hip / attention.hip / layernorm.hip / elementwise.hip, so the
// Python host issues one FFI call per pass and stays far ahead of the GPU.
#include "common.h"
#include "vlmo_hip.h"
#include <algorithm>
#include <map>
#include <vector>

namespace {
// VlmoEpilogue.relu bit 2: the fc1 epilogue saves GELU'(u) * dropout mask / (1 - p) in place of the pre-activation u, and the
// GELU-derivative epilogue of dgrad_fc2 multiplies by it
constexpr int GELU_DERIV = 4;


// vlmo_stack_bwd's fork / done event per deferred batch, of the calling thread, one pool per device (a process
// may drive several GPUs)
struct Events {
    std::vector<hipEvent_t> pool;
    hipEvent_t get(size_t i) {
        while (pool.size() <= i) {
            hipEvent_t e = nullptr;
            (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
            pool.push_back(e);
        }
        return pool[i];
    }
};
Events& events() {
    static thread_local std::map<int, Events> per_device;
    int dev = 0;
    (void)hipGetDevice(&dev);
    return per_device[dev];
}

inline const char* bp(const void* p, size_t row, size_t ld, size_t esz) { return (const char*)p + row * ld * esz; }
inline char* bp(void* p, size_t row, size_t ld, size_t esz) { return (char*)p + row * ld * esz; }

#define TRY(x)              \
    do {                    \
        int rc__ = (x);     \
        if (rc__) return rc__; \
    } while (0)

VlmoEpilogue epi() {
    VlmoEpilogue e{};
    e.inv_keep = 1.f;
    return e;
}

// forward of one block on `st` (vlmo_stack_fwd runs it per block)
int block_fwd(const VlmoBlockDesc* b, hipStream_t st) {
    VLMO_CHECK_ARG(b && b->x && b->x1 && b->x2, "vlmo_stack_fwd: null block buffers");
    VLMO_CHECK_ARG(b->n_experts >= 1 && b->n_experts <= 2 && b->n_attn >= 1 && b->n_attn <= 2, "vlmo_stack_fwd: bad counts");
    const int M = b->M, d = b->d, hid = b->hidden;
    TRY(vlmo_ln_fwd(b->x, b->n1w, b->n1b, b->y1, 0, b->mean1, b->rstd1, nullptr, M, d, b->eps, st));
    {
        VlmoEpilogue e = epi();
        e.out = b->qkv;
        e.ldo = 3 * d;
        e.bias = b->qkv_bias;
        TRY(vlmo_gemm_nt(VLMO_EPI_BIAS, VLMO_BF16, b->tile, b->y1, d, b->qkv_w, d, M, 3 * d, d, &e, st));
    }
    const float scale = 1.0f / sqrtf((float)(d / b->heads));
    for (int a = 0; a < b->n_attn; ++a)
        TRY(vlmo_attn_fwd(b->qkv, b->seg[a], b->nseq[a], b->keymask, b->ctx, b->lse[a], b->lse_stride[a], b->heads, d,
                          b->maxlen[a], scale, b->attn_drop_thresh, b->attn_inv_keep, b->seed + 11 + b->attn_seed_idx[a], b->attn_seq0[a], st));
    {
        VlmoEpilogue e = epi();
        e.out = b->x1;
        e.ldo = d;
        e.out2 = b->need_bwd ? b->zd1 : nullptr;
        e.ld2 = d;
        e.bias = b->proj_b;
        e.gamma = b->g1;
        e.resid = b->x;
        e.row_scale = b->rs1;
        e.row_index = b->row_index;
        e.drop_thresh = b->drop_thresh;
        e.inv_keep = b->inv_keep;
        e.seed = b->seed + 1;
        TRY(vlmo_gemm_nt(VLMO_EPI_RESID, VLMO_BF16, b->tile, b->ctx, d, b->proj_w, d, M, d, d, &e, st));
    }
    TRY(vlmo_ln_fwd(b->x1, b->n2w, b->n2b, b->y2, 0, b->mean2, b->rstd2, nullptr, M, d, b->eps, st));
    // expert FFNs: all experts of the block in ONE grouped launch per linear (row ranges, weights and biases
    // differ per expert; a launch costs at least one tile time, so per-expert launches of the 4 096 text rows
    // and the 12 608 image rows would cost two)
    const void *a1[4], *w1[4], *a2[4], *w2[4];
    int32_t rows[4];
    VlmoEpilogue e1[4], e2[4];
    for (int x = 0; x < b->n_experts; ++x) {
        const size_t r0 = b->exp_row0[x];
        rows[x] = b->exp_rows[x];
        a1[x] = bp(b->y2, r0, d, 2);
        w1[x] = b->w1[x];
        VlmoEpilogue& e = e1[x] = epi();
        e.out = bp(b->u, r0, hid, 2);
        e.out2 = bp(b->h, r0, hid, 2);
        e.ldo = e.ld2 = hid;
        e.bias = b->b1[x];
        e.drop_thresh = b->drop_thresh;
        e.inv_keep = b->inv_keep;
        e.seed = b->seed + 20 + 2 * x;
        e.relu = GELU_DERIV;         // `u` holds GELU'(u) * mask / (1 - p): see the backward's EPI_DGELU
        a2[x] = bp(b->h, r0, hid, 2);
        w2[x] = b->w2[x];
        VlmoEpilogue& f = e2[x] = epi();
        f.out = bp(b->x2, r0, d, 4);
        f.ldo = d;
        f.out2 = b->need_bwd ? bp(b->zd2, r0, d, 2) : nullptr;
        f.ld2 = d;
        f.bias = b->b2[x];
        f.gamma = b->g2;
        f.resid = (const float*)bp((const void*)b->x1, r0, d, 4);
        f.row_scale = b->row_index ? b->rs2 : (b->rs2 ? b->rs2 + r0 : nullptr);
        f.row_index = b->row_index ? b->row_index + r0 : nullptr;
        f.drop_thresh = b->drop_thresh;
        f.inv_keep = b->inv_keep;
        f.seed = b->seed + 21 + 2 * x;
    }
    TRY(vlmo_gemm_nt_grouped(VLMO_EPI_BIAS_GELU, VLMO_BF16, b->tile, b->n_experts, a1, d, w1, d, rows, hid, d, e1, st));
    TRY(vlmo_gemm_nt_grouped(VLMO_EPI_RESID, VLMO_BF16, b->tile, b->n_experts, a2, hid, w2, hid, rows, d, hid, e2, st));
    return 0;
}

}  // namespace

extern "C" int vlmo_side_stream_create(int low_priority, const uint32_t* cu_mask, int cu_mask_words, hipStream_t* out) {
    VLMO_CHECK_ARG(out, "vlmo_side_stream_create: null out");
    hipError_t rc;
    if (cu_mask && cu_mask_words > 0) {
        rc = hipExtStreamCreateWithCUMask(out, (uint32_t)cu_mask_words, cu_mask);
    } else {
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        rc = hipStreamCreateWithPriority(out, hipStreamNonBlocking, low_priority ? least : 0);
    }
    if (rc != hipSuccess) {
        vlmo_set_error("vlmo_side_stream_create: %s", hipGetErrorString(rc));
        return (int)rc;
    }
    return 0;
}

// ================================================================ whole block stacks in one call
// vlmo_stack_fwd / vlmo_stack_bwd run the blocks of one backbone pass (vlmo.py:402-411) from native code:
// one FFI call per pass and direction.  The backward enqueues the activation-gradient chains of all blocks
// back to back on the caller's stream and DEFERS every block's parameter-gradient work -- the four to six
// weight-gradient GEMMs and all bias / layer-scale / LayerNorm-weight column sums -- to the side stream in
// batches of `wgrad_batch` blocks: ONE vlmo_gemm_tn_multi launch (216 output tiles for two VLMo-Base blocks:
// the chip is full without splitting the token dimension) and ONE vlmo_colwork_multi launch per batch.
namespace {

struct Deferred {
    std::vector<VlmoTnProblem> tn;
    std::vector<VlmoColJob> col;
    std::vector<int> blocks;
    bool store = false;         // weight-gradient matrices are written, not accumulated (VlmoStackDesc.wgrad_store)
};

// a launcher that had nothing to fold leaves the job empty
void push_col(Deferred& D, const VlmoColJob& j) {
    if (j.src && j.rows > 0) D.col.push_back(j);
}
void push_tn(Deferred& D, const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N1, int N2) {
    D.tn.push_back(VlmoTnProblem{A, B, C, lda, ldb, ldc, M, N1, N2, 1.f, D.store ? 0 : 1});
}

// Column workspace of one block of vlmo_stack_bwd (VlmoBlockDesc.ws_main), offsets in floats.  THE definition: the
// chain below takes its pointers from it and vlmo_stack_bwd_ws_bytes() is its `total`.  Sized for the largest block the
// descriptor allows -- two experts, norm1 fused with the FFN branch of the block below -- whatever the block at hand is.
struct StackWs {
    int64_t ln2;        // norm2 + attention residual branch: [workgroups][4d] partial rows (two fold slots)
    int64_t resid[2];   // FFN residual branch of expert x: [workgroups][2d] (one fold slot each)
    int64_t ln1;        // norm1 (+ FFN residual branch of the block below): [workgroups][2d or 4d] (two fold slots)
    int64_t colpart;    // fc1 bias: column partials of the DGELU epilogue, [ceil(rows / 16)][hidden] per expert, expert 1
                        // behind expert 0: ceil(a / 16) + ceil(b / 16) <= ceil(M / 16) + 1 rows for a + b <= M
    int64_t qv;         // q / v bias: per-sequence dq | dv column sums of the attention backward, [sequences][2d]
    int64_t total;
    int64_t slot;       // one fold slot: at most VLMO_MAX_PARTIAL_BLOCKS partial rows of 2d columns
};
StackWs stack_ws_layout(int M, int d, int hidden, int max_seqs) {
    StackWs w{};
    w.slot = reduce_ws_need(2 * d) / 4;
    w.ln2 = 0;
    w.resid[0] = w.ln2 + 2 * w.slot;
    w.resid[1] = w.resid[0] + w.slot;
    w.ln1 = w.resid[1] + w.slot;
    w.colpart = w.ln1 + 2 * w.slot;
    w.qv = w.colpart + (int64_t)((M + 15) / 16 + 1) * hidden;
    w.total = w.qv + (int64_t)max_seqs * 2 * d;
    return w;
}
int block_seqs(const VlmoBlockDesc* b) {
    int n = 0;
    for (int a = 0; a < b->n_attn; ++a) n += b->nseq[a];
    return n;
}

// what block_dgrad_chain relies on, checked for all blocks before vlmo_stack_bwd enqueues anything
int check_block_bwd(const VlmoBlockDesc* b, int i) {
    VLMO_CHECK_ARG(b->dx2 && b->dx1 && b->dx0, "vlmo_stack_bwd: block %d: null gradient buffers", i);
    VLMO_CHECK_ARG(b->n_experts >= 1 && b->n_experts <= 2 && b->n_attn >= 1 && b->n_attn <= 2,
                   "vlmo_stack_bwd: block %d: 1..2 experts and attention launches per block", i);
    VLMO_CHECK_ARG(b->M > 0 && b->exp_rows[0] >= 0 && (b->n_experts == 1 || b->exp_rows[1] >= 0) &&
                       (int64_t)b->exp_rows[0] + (b->n_experts == 2 ? b->exp_rows[1] : 0) <= b->M,
                   "vlmo_stack_bwd: block %d: expert rows exceed M = %d", i, b->M);
    const int64_t need = stack_ws_layout(b->M, b->d, b->hidden, block_seqs(b)).total * 4;
    VLMO_CHECK_ARG(b->ws_main && b->ws_bytes >= need,
                   "vlmo_stack_bwd: block %d: column workspace of %lld bytes is too small: need %lld bytes = "
                   "vlmo_stack_bwd_ws_bytes(%d, %d, %d, %d)",
                   i, (long long)b->ws_bytes, (long long)need, b->M, b->d, b->hidden, block_seqs(b));
    return 0;
}

// activation-gradient chain of one block on `st`; parameter-gradient work is appended to D.
// `below` = the block processed next (the one under this one in the stack), or NULL: when its FFN residual branch can
// take its incoming gradient straight from this block's last kernel, norm1's backward and that branch's backward run as
// ONE kernel (the 51 MB fp32 gradient is not re-read) and *fused_below is set; the chain of `below` is then started
// with skip_resid.
int block_dgrad_chain(const VlmoBlockDesc* b, hipStream_t st, Deferred& D, const VlmoBlockDesc* below, bool skip_resid,
                      bool* fused_below) {
    const int M = b->M, d = b->d, hid = b->hidden;
    const int nseq_all = block_seqs(b);
    const StackWs W = stack_ws_layout(M, d, hid, nseq_all);
    const int64_t slot_bytes = W.slot * 4;
    float* const ws = b->ws_main;
    const void *ag[4], *wg[4], *af[4], *wf[4];
    int32_t rows[4];
    VlmoEpilogue eg[4], ef[4];
    float* colpart = ws + W.colpart;
    for (int x = 0; x < b->n_experts; ++x) {
        const size_t r0 = b->exp_row0[x];
        const int n = rows[x] = b->exp_rows[x];
        if (!skip_resid) {
            VlmoColJob fold{};
            TRY(resid_bwd_launch(b->dx2 + r0 * d, bp(b->zd2, r0, d, 2), b->g2,
                                 b->row_index ? b->rs2 : (b->rs2 ? b->rs2 + r0 : nullptr),
                                 b->row_index ? b->row_index + r0 : nullptr, bp(b->dz2, r0, d, 2), b->dg2, b->db2[x], n, d,
                                 b->drop_thresh, b->inv_keep, b->seed + 21 + 2 * x, ws + W.resid[x], slot_bytes, &fold, st));
            push_col(D, fold);
        }
        ag[x] = bp(b->dz2, r0, d, 2);
        wg[x] = b->w2T[x];
        VlmoEpilogue& e = eg[x] = epi();
        e.out = bp(b->du, r0, hid, 2);
        e.ldo = hid;
        e.aux = bp(b->u, r0, hid, 2);
        e.ld2 = hid;
        e.drop_thresh = b->drop_thresh;
        e.inv_keep = b->inv_keep;
        e.seed = b->seed + 20 + 2 * x;
        e.relu = GELU_DERIV;
        // fc1 bias gradient: the DGELU epilogue leaves column-sum partials (one row per 16 output rows, see
        // VlmoEpilogue.colpart); they join the block's other column folds
        if (b->db1[x]) {
            const int nblk16 = (n + 15) / 16;
            e.colpart = colpart;
            push_col(D, fold_job(colpart, hid, nblk16, hid, hid, b->db1[x]));
            colpart += (int64_t)nblk16 * hid;
        }
        af[x] = bp(b->du, r0, hid, 2);
        wf[x] = b->w1T[x];
        VlmoEpilogue& f = ef[x] = epi();
        f.out = bp(b->dy2, r0, d, 2);
        f.ldo = d;
        push_tn(D, bp(b->dz2, r0, d, 2), d, bp(b->h, r0, hid, 2), hid, b->dw2[x], hid, n, d, hid);
        push_tn(D, bp(b->du, r0, hid, 2), hid, bp(b->y2, r0, d, 2), d, b->dw1[x], d, n, hid, d);
    }
    TRY(vlmo_gemm_nt_grouped(VLMO_EPI_DGELU, VLMO_BF16, b->tile, b->n_experts, ag, d, wg, d, rows, hid, d, eg, st));
    TRY(vlmo_gemm_nt_grouped(VLMO_EPI_BIAS, VLMO_BF16, b->tile, b->n_experts, af, hid, wf, hid, rows, d, hid, ef, st));
    {
        VlmoColJob fold{};
        TRY(ln_bwd_fold(b->dy2, b->x1, b->n2w, b->mean2, b->rstd2, b->dx2, b->dx1, b->dn2w, b->dn2b, b->zd1, b->g1, b->rs1,
                        b->row_index, b->dz1, b->dg1, b->dproj_b, b->drop_thresh, b->inv_keep, b->seed + 1, M, d, ws + W.ln2,
                        2 * slot_bytes, &fold, st));
        push_col(D, fold);
    }
    {
        VlmoEpilogue e = epi();
        e.out = b->dctx;
        e.ldo = d;
        TRY(vlmo_gemm_nt(VLMO_EPI_BIAS, VLMO_BF16, b->tile, b->dz1, d, b->proj_wT, d, M, d, d, &e, st));
    }
    const float scale = 1.0f / sqrtf((float)(d / b->heads));
    // q_bias / v_bias gradient = column sums of the q and v thirds of dqkv (the k third of the bias is a constant zero,
    // vlmo.py:71-75, and its gradient vanishes anyway: the soft-max is invariant to a shift of the scores along the
    // keys).  The attention backward leaves them per sequence ([sequences][2d]) and the batched column kernel folds
    // 64-128 rows instead of reading 51 MB of dqkv again.
    float* const qvsum = ws + W.qv;
    for (int a = 0, s0 = 0; a < b->n_attn; s0 += b->nseq[a], ++a)
        TRY(vlmo_attn_bwd(b->qkv, b->ctx, b->dctx, b->lse[a], b->lse_stride[a], b->seg[a], b->nseq[a], b->keymask,
                          b->dqkv, qvsum + (size_t)s0 * 2 * d, b->heads, d, b->maxlen[a], scale, b->attn_drop_thresh,
                          b->attn_inv_keep, b->seed + 11 + b->attn_seed_idx[a], b->attn_seq0[a], st));
    push_tn(D, b->dz1, d, b->ctx, d, b->dproj_w, d, M, d, d);
    push_tn(D, b->dqkv, 3 * d, b->y1, d, b->dqkv_w, d, M, 3 * d, d);
    push_col(D, fold_job(qvsum, 2 * d, nseq_all, 2 * d, d, b->dqkv_b, b->dqkv_b + 2 * d));
    {
        VlmoEpilogue e = epi();
        e.out = b->dy1;
        e.ldo = d;
        TRY(vlmo_gemm_nt(VLMO_EPI_BIAS, VLMO_BF16, b->tile, b->dqkv, 3 * d, b->qkv_wT, 3 * d, M, d, 3 * d, &e, st));
    }
    const VlmoBlockDesc* n = below;
    *fused_below = n && n->M == M && n->d == d && n->dx2 == b->dx0 && n->zd2 && n->dz2 && n->exp_row0[0] == 0 &&
                   (n->n_experts == 1 ? n->exp_rows[0] == M
                                      : (n->exp_row0[1] == n->exp_rows[0] && n->exp_rows[0] + n->exp_rows[1] == M));
    VlmoColJob fold{};
    if (*fused_below) {
        const int seg = n->n_experts == 1 ? M : n->exp_row0[1];
        float* wsf = ws + W.ln1;        // [workgroups][4d]
        int nb0 = 0;
        TRY(ln_resid_seg_bwd(b->dy1, b->x, b->n1w, b->mean1, b->rstd1, b->dx1, b->dx0, b->dn1w, b->dn1b, n->zd2, n->g2,
                             n->rs2, n->row_index, n->dz2, n->dg2, n->drop_thresh, n->inv_keep, n->seed + 21, n->seed + 23,
                             seg, M, d, wsf, 2 * slot_bytes, &fold, &nb0, st));
        push_col(D, fold);
        // the FFN bias gradients of the block below: columns [3d, 4d) of the partial rows of each segment
        if (n->db2[0]) push_col(D, fold_job(wsf + 3 * d, 4 * d, nb0, d, d, n->db2[0]));
        if (n->n_experts == 2 && n->db2[1])
            push_col(D, fold_job(wsf + 3 * d + (size_t)nb0 * 4 * d, 4 * d, fold.rows - nb0, d, d, n->db2[1]));
    } else {
        TRY(ln_bwd_fold(b->dy1, b->x, b->n1w, b->mean1, b->rstd1, b->dx1, b->dx0, b->dn1w, b->dn1b, nullptr, nullptr, nullptr,
                        nullptr, nullptr, nullptr, nullptr, 0, 1.f, 0, M, d, ws + W.ln1, slot_bytes, &fold, st));
        push_col(D, fold);
    }
    return 0;
}

}  // namespace

extern "C" int64_t vlmo_stack_bwd_ws_bytes(int M, int d, int hidden, int max_seqs) {
    return stack_ws_layout(M, d, hidden, max_seqs).total * 4;
}

extern "C" int vlmo_stack_fwd(const VlmoStackDesc* s, hipStream_t st) {
    VLMO_CHECK_ARG(s && s->blocks && s->n_blocks >= 1, "vlmo_stack_fwd: empty stack");
    for (int i = 0; i < s->n_blocks; ++i)
        if (int rc = block_fwd(&s->blocks[i], st)) return rc;
    return 0;
}

extern "C" int vlmo_stack_bwd(const VlmoStackDesc* s, hipStream_t st) {
    VLMO_CHECK_ARG(s && s->blocks && s->n_blocks >= 1, "vlmo_stack_bwd: empty stack");
    const int nb = s->n_blocks;
    for (int i = 0; i < nb; ++i) TRY(check_block_bwd(&s->blocks[i], i));
    const int batch = s->wgrad_batch >= 1 ? s->wgrad_batch : 1;
    const int nsets = s->n_tmp_sets >= 1 ? s->n_tmp_sets : 1;
    hipStream_t side = s->side_stream ? s->side_stream : st;
    const bool two = side != st;
    VLMO_CHECK_ARG(!two || nsets > batch || nb <= nsets,
                   "vlmo_stack_bwd: %d temporary sets cannot cover deferred batches of %d blocks", nsets, batch);
    Events& ev = events();
    Deferred D;
    D.store = s->wgrad_store != 0;
    std::vector<int> batch_of(nb, -1);
    int n_batches = 0, waited_upto = -1;
    auto flush = [&]() -> int {
        if (D.blocks.empty()) return 0;
        if (two) {
            hipEvent_t f = ev.get(2 * n_batches);
            (void)hipEventRecord(f, st);
            (void)hipStreamWaitEvent(side, f, 0);
        }
        // longest reductions first: with more tiles than CUs the short ones back-fill
        std::stable_sort(D.tn.begin(), D.tn.end(), [](const VlmoTnProblem& a, const VlmoTnProblem& b) { return a.M > b.M; });
        TRY(vlmo_gemm_tn_multi(VLMO_BF16, D.tn.data(), (int)D.tn.size(), side));
        TRY(vlmo_colwork_multi(VLMO_BF16, D.col.data(), (int)D.col.size(), side));
        if (two) (void)hipEventRecord(ev.get(2 * n_batches + 1), side);
        if (s->grad_ready)
            for (int i : D.blocks)
                if (s->grad_ready[i]) (void)hipEventRecord((hipEvent_t)s->grad_ready[i], side);
        ++n_batches;
        D.tn.clear();
        D.col.clear();
        D.blocks.clear();
        return 0;
    };
    auto set_free = [&](int kk) -> int {
        // block kk (processing order) reuses the temporaries of the block processed nsets steps earlier: that block's
        // deferred work must be done
        if (!two || kk < nsets || kk >= nb) return 0;
        int need = batch_of[kk - nsets];
        if (need < 0 || need >= n_batches) {
            TRY(flush());
            need = n_batches - 1;
        }
        if (need >= 0 && need > waited_upto) {
            (void)hipStreamWaitEvent(st, ev.get(2 * need + 1), 0);
            waited_upto = need;
        }
        return 0;
    };
    bool skip_resid = false;
    for (int k = 0; k < nb; ++k) {
        const int i = nb - 1 - k;
        TRY(set_free(k));
        TRY(set_free(k + 1));       // the last kernel of this chain may already write dz2 of the block below
        bool fused = false;
        TRY(block_dgrad_chain(&s->blocks[i], st, D, i > 0 ? &s->blocks[i - 1] : nullptr, skip_resid, &fused));
        skip_resid = fused;
        D.blocks.push_back(i);
        batch_of[k] = n_batches;
        if ((int)D.blocks.size() >= batch || k == nb - 1) TRY(flush());
    }
    if (two && n_batches > 0) (void)hipStreamWaitEvent(st, ev.get(2 * (n_batches - 1) + 1), 0);
    return 0;
}

extern "C" int vlmo_event_create(void** out) {
    VLMO_CHECK_ARG(out, "vlmo_event_create: null out");
    hipEvent_t e = nullptr;
    hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (rc != hipSuccess) {
        vlmo_set_error("vlmo_event_create: %s", hipGetErrorString(rc));
        return (int)rc;
    }
    *out = e;
    return 0;
}
extern "C" int vlmo_event_destroy(void* ev) { return ev ? (int)hipEventDestroy((hipEvent_t)ev) : 0; }
extern "C" int vlmo_stream_wait_event(hipStream_t stream, void* ev) {
    VLMO_CHECK_ARG(ev, "vlmo_stream_wait_event: null event");
    return (int)hipStreamWaitEvent(stream, (hipEvent_t)ev, 0);
}
