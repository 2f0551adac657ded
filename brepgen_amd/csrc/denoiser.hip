// Whole-net forward of the four BrepGen denoisers (network.py:1107-1126, 1176-1200, 1257-1286, 1357-1393),
// enqueued on one stream from ONE C-ABI call: batch-first [M = B*N, 768] layout end to end (the reference's
// seq-first permutes -- 38 % of its CPU time -- do not exist here), residual stream in fp32 (fp32 mode, unfolded weights) or as a
// split pair of 16-bit planes with the LayerNorms folded into the next GEMM (16-bit modes), activations in the compute dtype,
// step-invariant conditioning embeds cached across denoising steps.  run() is the call, stage by stage; bg_embed_mlp_fwd and
// bg_encoder_layer_fwd expose two of its pieces.  (Error plumbing, bg_tune and the profiler: runtime.hip.)
#include "bg_common.h"
#include <mutex>

namespace bg {

__global__ void expand_mask_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, size_t n, int E) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = in[i / E];
}

static inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct Workspace {
    size_t off_x, off_h, off_r, off_small, off_f, off_mask, off_stats, off_rows, off_slots, total;
    int M, F;
    int Mrow;           // row capacity of the token buffers: M, or 64 rows per sample where a ragged batch may run slot-packed
};

// Slot-packed variable-length execution (compact.hip: compact_rows_paired + the fused QKV / attention launch): nets whose samples
// have at most 64 tokens, 16-bit modes.  Its rows are 64-row slots of one or two samples -- up to 64 B of them, more than the
// padded batch when nothing can be paired -- so the token buffers of these nets are planned for 64 rows per sample.
static inline bool slot_packing_applies(int net, int B, int S, int E, int dtype) {
    return net == BG_SURFZ && E == 1 && S <= 64 && dtype != BG_F32 && B <= 8192;
}

static Workspace plan(int net, int B, int S, int E, int dtype) {
    Workspace w{};
    const size_t es = (dtype == BG_F32) ? 4 : 2;
    w.M = B * S * E;
    w.F = B * S;
    const bool slots = slot_packing_applies(net, B, S, E, dtype);
    // worst case of the slot-packed layout: S <= 32 -- any two samples fit one slot, at most ceil(B / 2) slots; otherwise nothing
    // may pair: one slot per sample
    const int slot_rows = 64 * (S <= 32 ? (B + 1) / 2 : B);
    w.Mrow = slots && slot_rows > w.M ? slot_rows : w.M;
    const size_t Fr = slots ? (size_t)w.Mrow : (size_t)w.F;        // (the per-face conditioning embed of SurfZNet runs on the compact rows)
    size_t o = 0;
    w.off_x = o; o += align_up((size_t)w.Mrow * 768 * 4);
    w.off_h = o; o += align_up((size_t)w.Mrow * 768 * es);
    w.off_r = o; o += align_up((size_t)w.Mrow * 2304 * es);
    w.off_small = o; o += align_up((size_t)(4 * B + B) * 768 * 4);      // sincos, t0, t1(as fp32 worst case), temb, cvec
    w.off_f = o; o += (net != BG_SURFPOS) ? align_up(Fr * 768 * 4) : 0;
    w.off_mask = o; o += (net == BG_EDGEPOS) ? align_up((size_t)w.M) : 0;
    w.off_stats = o; o += (dtype != BG_F32) ? align_up((size_t)w.Mrow * 12 * 2 * 4) : 0;   // LayerNorm-fold row partials
    w.off_rows = o; o += (net != BG_SURFPOS) ? align_up((size_t)(B + 2 + P256_RULE_ENTRIES) * 4) + align_up((size_t)w.Mrow * 4) : 0;   // var-len: offsets + GEMM partition table, row map
    w.off_slots = o; o += slots ? align_up((size_t)4 * B * 4) : 0;       // slot-packed: (n_a, n_b) per slot, first sample per slot, counts
    w.total = o;
    return w;
}

struct Ctx {
    const bg_denoiser_weights* w;
    hipStream_t s;
    int dtype;
    unsigned char* ws;
    Workspace p;
    float* X;
    void* H;
    void* R;
    // 16-bit compute dtypes with folded LayerNorms: the residual stream lives as two 16-bit planes x = XH + XL in the
    // X region (same bytes as fp32), XH doubles as the A operand of the QKV / FFN1 GEMMs, and the producers of x
    // (token embeds, out-proj, FFN2) leave per-row (sum, sum of squares) partials in `stats`.
    bool fold = false;
    void* XH = nullptr;
    void* XL = nullptr;
    float* stats = nullptr;
    // variable-length execution: valid tokens compacted into rows 0 .. *m_dev-1 (csrc/compact.hip)
    const int* m_dev = nullptr;       // device-side row count (offsets[B])
    const int* src_row = nullptr;     // compact row -> padded-layout token index
    const int* offsets = nullptr;     // per-sample first row, [B+1]
    const int* rule = nullptr;        // 256 / 128 kernel partition of the GEMM launches for this row count (compact.hip)
    const int* slot_desc = nullptr;   // slot-packed batch: (n_a, n_b) per 64-row slot (compact_rows_paired)
    double rows_hint = 0.0, pairs_hint = 0.0;   // host-side estimates: GEMM kernel choice + profiler accounting (brepgen_hip.h)
    double rows_plan = 0.0;                     // the row count the caller knows exactly (0 = not): launch plan only
    int concurrent = 0;               // sibling sample groups are in flight on forked streams (n_split > 1)
    // the call: B samples of N tokens, M = row bound of every token-wise launch (the stand-alone pieces set what they use)
    const bg_denoiser_inputs* in = nullptr;
    int net = 0, B = 0, N = 1, E = 1, M = 0;
    bool varlen = false;              // the valid tokens run compacted
    bool paired = false;              // ... in 64-row slots of one or two samples, through the fused QKV / attention launch
    bool fused_qkv = false;           // dense run: QKV + attention as one launch
    const uint8_t* key_pad = nullptr; // [B, N] key-padding mask of the attention launches (null: every row is a valid key)
    float* cvec = nullptr;            // [B, 768] time (+ class) embedding per sample
};

// The row count of a token-wise GEMM -- all five fields, set here and nowhere else.  Forgetting one still computes the right
// result (every launch plan is correct for any row count) on a different kernel plan, which no parity test sees.
// launch_plan = false: the count and its estimate only -- the embed MLPs' GEMMs, whose kernel choice has never looked at the rest.
static void token_rows(const Ctx& c, GemmArgs& g, bool launch_plan = true) {
    g.m_dev = c.m_dev; g.rows_hint = c.rows_hint;
    if (launch_plan) { g.rule_table = c.rule; g.rows_plan = c.rows_plan; g.concurrent = c.concurrent; }
}

struct Addend { const float* rows = nullptr; int ld = 0; int div = 1; };   // fp32 rows [*, ld]: output row r adds rows[r / div]
// TO_STREAM: the result goes to the token stream X -- fp32 rows (out = c.X, and add == c.X accumulates), or, in
// fold mode, the split pair (XH, XL) with row statistics (accumulating = the stream is the addend)
// TOK: the rows are tokens.  In a variable-length run they are the COMPACT rows (count on the device): with GATHER the inputs
// are gathered through c.src_row, with MAP_ADD / MAP_ADD2 that broadcast addend is looked up through it (indexed by the padded
// token index / div), and with SCATTER the result rows go back to the padded layout.
enum EmbedOpt : unsigned { TO_STREAM = 1, TOK = 2, GATHER = 4, MAP_ADD = 8, MAP_ADD2 = 16, SCATTER = 32 };

// Linear(k,768)+b -> LN -> SiLU -> Linear(768,n)+b (+adds) ; x fp32 rows (lda), or activations in compute dtype for fc_out
static int embed_mlp(Ctx& c, const bg_mlp_weights& m, const void* x, int lda, int rows, float* out, int ldc, Addend add = {},
                     Addend add2 = {}, unsigned opt = 0) {
    int rc;
    const bool vl = (opt & TOK) && c.m_dev != nullptr;
    if (m.w0_mfma && m.w0_dtype == BG_F32 && embed_ln_silu_supported(m.k_in)) {
        // input embeds (k = 6 / 12 / 48): Linear + LayerNorm + SiLU in one kernel, nothing but the result written
        rc = embed_ln_silu(reinterpret_cast<const float*>(x), lda, rows, m.k_in, m.w0_mfma, m.b0, m.ln_g, m.ln_b, c.H,
                           c.dtype, 1e-5f, c.s, vl ? c.m_dev : nullptr, (vl && (opt & GATHER)) ? c.src_row : nullptr, vl ? c.rows_hint : 0.0);
        if (rc) return rc;
    } else {
        BG_REQUIRE(!(vl && (opt & GATHER)), BG_E_ARG, "bg_denoiser_fwd: variable-length execution needs the fused input embeds (w0_mfma)");
        float* t0 = reinterpret_cast<float*>(c.R);
        GemmArgs g1 = linear(x, lda, m.w0, m.b0, t0, 768, rows, 768, 768, m.k_in, BG_F32);
        g1.gemv_ok = (&m == &c.w->time_embed);                    // one row per distinct timestep
        if (vl) token_rows(c, g1, /*launch_plan=*/false);
        rc = gemm(g1, m.w0_dtype, c.s);
        if (rc) return rc;
        rc = layernorm768(t0, m.ln_g, m.ln_b, c.H, c.dtype, rows, 1e-5f, /*silu=*/1, c.s, vl ? c.m_dev : nullptr, vl ? c.rows_hint : 0.0);
        if (rc) return rc;
    }
    GemmArgs g2 = linear(c.H, 768, m.w3, m.b3, out, ldc, rows, m.n_out, m.n_out_pad, 768, BG_F32);
    add_rows(g2, add.rows, add.ld, add.div);
    add2_rows(g2, add2.rows, add2.ld, add2.div);
    if (vl) token_rows(c, g2, /*launch_plan=*/false);
    if (vl && (opt & (MAP_ADD | MAP_ADD2 | SCATTER))) map_rows(g2, c.src_row, opt & MAP_ADD, opt & MAP_ADD2, opt & SCATTER);
    if ((opt & TO_STREAM) && c.fold) {
        g2.out = c.XH; g2.out_dtype = c.dtype;
        split_out(g2, c.XL, c.stats);
        if (add.rows == c.X) {                                    // accumulate into the stream
            add_rows(g2, nullptr, 0, 1);
            split_residual_in(g2, c.XH, c.XL, 768);
        }
    }
    return gemm(g2, c.dtype, c.s);
}

// One pre-LN encoder layer on the fp32 residual stream c.X, in place: LayerNorm kernels + unfolded weights (fp32 mode, and 16-bit
// weights without the fold's column sums).  bg_encoder_layer_fwd is this routine with no variable-length context.
static int encoder_layer_unfolded(const Ctx& c, const bg_layer_weights& L) {
    int rc;
    const int M = c.M;
    if ((rc = layernorm768(c.X, L.ln1_g, L.ln1_b, c.H, c.dtype, M, 1e-5f, /*silu=*/0, c.s, c.m_dev, c.rows_hint))) return rc;
    GemmArgs qkv = linear(c.H, 768, L.w_qkv, L.b_qkv, c.R, 2304, M, 2304, 2304, 768, c.dtype);
    token_rows(c, qkv);
    if ((rc = gemm(qkv, c.dtype, c.s))) return rc;
    if ((rc = attention(c.R, c.key_pad, c.H, c.B, c.N, c.dtype, c.s, c.offsets, c.pairs_hint, c.rows_hint))) return rc;
    GemmArgs op = linear(c.H, 768, L.w_o, L.b_o, c.X, 768, M, 768, 768, 768, BG_F32);
    add_rows(op, c.X, 768, 1);
    token_rows(c, op);
    if ((rc = gemm(op, c.dtype, c.s))) return rc;
    if ((rc = layernorm768(c.X, L.ln2_g, L.ln2_b, c.H, c.dtype, M, 1e-5f, /*silu=*/0, c.s, c.m_dev, c.rows_hint))) return rc;
    GemmArgs f1 = linear(c.H, 768, L.w_1, L.b_1, c.R, 1024, M, 1024, 1024, 768, c.dtype, BG_ACT_RELU);
    token_rows(c, f1);
    if ((rc = gemm(f1, c.dtype, c.s))) return rc;
    GemmArgs f2 = linear(c.R, 1024, L.w_2, L.b_2, c.X, 768, M, 768, 768, 1024, BG_F32);
    add_rows(f2, c.X, 768, 1);
    token_rows(c, f2);
    return gemm(f2, c.dtype, c.s);
}

// The same layer on the split stream x = XH + XL (16-bit modes).  LN1 / LN2 are folded: QKV and FFN1 read the raw 16-bit rows XH
// and normalise in their epilogue; out-proj and FFN2 add the split residual in place and leave the next fold's row statistics.
static int encoder_layer_folded(const Ctx& c, const bg_layer_weights& L) {
    int rc;
    const int M = c.M;
    if (c.paired) {
        // ragged batch, slot-packed: one or two whole samples per 64-row slot (qkv_attn.hip, PAIR)
        if ((rc = qkv_attention_paired(c.XH, L.w_qkv, L.b_qkv, L.qkv_colsum, c.stats, c.H, nullptr, c.m_dev, c.slot_desc,
                                       c.B < (M + 63) / 64 ? c.B : (M + 63) / 64, M, c.dtype,
                                       1e-5f, c.s, c.rows_hint, c.pairs_hint))) return rc;
    } else if (c.fused_qkv) {
        // short, equally long sequences (SurfPosNet; SurfZNet executed densely): q|k|v never leave the CU (qkv_attn.hip; bit-identical)
        if ((rc = qkv_attention(c.XH, L.w_qkv, L.b_qkv, L.qkv_colsum, c.stats, c.H, c.key_pad, c.B, c.N, c.dtype, 1e-5f, c.s))) return rc;
    } else {
        GemmArgs qkv = linear(c.XH, 768, L.w_qkv, L.b_qkv, c.R, 2304, M, 2304, 2304, 768, c.dtype);
        ln_fold_in(qkv, c.stats, L.qkv_colsum);
        token_rows(c, qkv);
        if ((rc = gemm(qkv, c.dtype, c.s))) return rc;
        if ((rc = attention(c.R, c.key_pad, c.H, c.B, c.N, c.dtype, c.s, c.offsets, c.pairs_hint, c.rows_hint))) return rc;
    }
    GemmArgs op = linear(c.H, 768, L.w_o, L.b_o, c.XH, 768, M, 768, 768, 768, c.dtype);
    split_out(op, c.XL, c.stats);
    split_residual_in(op, c.XH, c.XL, 768);
    token_rows(c, op);
    if ((rc = gemm(op, c.dtype, c.s))) return rc;
    if (L.w_1f && L.w_2f && g_tune[BG_TUNE_FFN_FUSED] != 1) {
        // FFN1 + ReLU + FFN2 + residual as one launch: the [M, 1024] hidden tensor stays in the CU's LDS (ffn_fused.hip; bit-identical)
        FfnArgs ff{c.XH, c.XL, c.stats, L.w_1f, L.b_1, L.w1_colsum, L.w_2f, L.b_2, M, M, c.m_dev, 1e-5f};      // (statistics stride = the launch's row bound, as the GEMMs')
        BG_REQUIRE(ffn_fused_eligible(ff, c.dtype), BG_E_ARG, "bg_denoiser_fwd: w_1f / w_2f given, but the fused FFN launch does not apply");
        return ffn_fused(ff, c.dtype, c.s, c.rows_hint);
    }
    GemmArgs f1 = linear(c.XH, 768, L.w_1, L.b_1, c.R, 1024, M, 1024, 1024, 768, c.dtype, BG_ACT_RELU);
    ln_fold_in(f1, c.stats, L.w1_colsum);
    token_rows(c, f1);
    if ((rc = gemm(f1, c.dtype, c.s))) return rc;
    GemmArgs f2 = linear(c.R, 1024, L.w_2, L.b_2, c.XH, 768, M, 768, 768, 1024, c.dtype);
    split_out(f2, c.XL, c.stats);
    split_residual_in(f2, c.XH, c.XL, 768);
    token_rows(c, f2);
    return gemm(f2, c.dtype, c.s);
}

// ---- the stages of one whole-net forward, in the order run() calls them ---------------------------------------------------

static int check_args(const bg_denoiser_weights* w, const bg_denoiser_inputs* in, const float* eps_out, const void* workspace) {
    const int net = w->net, B = in->B, S = in->S, E = (net >= BG_EDGEPOS) ? in->E : 1;
    BG_REQUIRE(net >= BG_SURFPOS && net <= BG_EDGEZ, BG_E_ARG, "bg_denoiser_fwd: bad net id %d", net);
    BG_REQUIRE(w->dtype == BG_BF16 || w->dtype == BG_F16 || w->dtype == BG_F32, BG_E_DTYPE, "bg_denoiser_fwd: compute dtype %d", w->dtype);
    BG_REQUIRE(B > 0 && S > 0 && E > 0, BG_E_SHAPE, "bg_denoiser_fwd: empty shape B=%d S=%d E=%d", B, S, E);
    BG_REQUIRE(in->n_timesteps == 1 || in->n_timesteps == B, BG_E_SHAPE, "bg_denoiser_fwd: n_timesteps must be 1 or B");
    BG_REQUIRE(in->x && in->timesteps && eps_out && workspace, BG_E_ARG, "bg_denoiser_fwd: null pointer");
    BG_REQUIRE(w->n_layer >= 0 && w->n_layer <= BG_MAX_LAYERS, BG_E_ARG, "bg_denoiser_fwd: n_layer");
    BG_REQUIRE((w->class_embed == nullptr) || in->class_label, BG_E_ARG, "bg_denoiser_fwd: class_label required (use_cf)");
    if (net != BG_SURFPOS) BG_REQUIRE(in->surf_pos, BG_E_ARG, "bg_denoiser_fwd: surf_pos missing");
    if (net >= BG_EDGEPOS) BG_REQUIRE(in->surf_z, BG_E_ARG, "bg_denoiser_fwd: surf_z missing");
    if (net == BG_EDGEZ) BG_REQUIRE(in->edge_pos, BG_E_ARG, "bg_denoiser_fwd: edge_pos missing");
    BG_REQUIRE(((uintptr_t)workspace & 255) == 0, BG_E_ALIGN, "bg_denoiser_fwd: workspace must be 256-byte aligned");
    return 0;
}

// the call's shape, its execution mode (variable-length / slot-packed / LayerNorm fold) and the workspace regions
static int bind_workspace(Ctx& c, const bg_denoiser_weights* w, const bg_denoiser_inputs* in, void* workspace, size_t ws_bytes) {
    const int net = w->net, B = in->B, S = in->S, E = (net >= BG_EDGEPOS) ? in->E : 1;
    c.w = w; c.in = in; c.dtype = w->dtype;
    c.net = net; c.B = B; c.E = E; c.N = S * E;
    c.p = plan(net, B, S, E, w->dtype);
    BG_REQUIRE(ws_bytes >= c.p.total, BG_E_WORKSPACE, "bg_denoiser_fwd: workspace %zu < %zu bytes", ws_bytes, c.p.total);
    c.ws = reinterpret_cast<unsigned char*>(workspace);
    c.X = reinterpret_cast<float*>(c.ws + c.p.off_x);
    c.H = c.ws + c.p.off_h;
    c.R = c.ws + c.p.off_r;
    c.cvec = reinterpret_cast<float*>(c.ws + c.p.off_small) + (size_t)4 * B * 768;
    // variable-length execution: the valid tokens are compacted (row count stays on the device)
    c.varlen = in->varlen != 0 && in->mask != nullptr && net != BG_SURFPOS;
    // ragged batches of short sequences: slot-packed rows + the fused QKV / attention launch (BG_TUNE_QKV_ATTN = 1: dense packing +
    // GEMM + attention, the bit-equality baseline)
    c.paired = c.varlen && slot_packing_applies(net, B, S, E, w->dtype) && w->n_layer > 0 && w->layers[0].qkv_colsum != nullptr &&
               g_tune[BG_TUNE_QKV_ATTN] != 1;
    c.M = c.paired ? c.p.Mrow : c.p.M;
    c.fold = w->dtype != BG_F32 && w->n_layer > 0 && w->layers[0].qkv_colsum != nullptr;
    if (c.fold) {
        for (int li = 0; li < w->n_layer; ++li)
            BG_REQUIRE(w->layers[li].qkv_colsum && w->layers[li].w1_colsum, BG_E_ARG,
                       "bg_denoiser_fwd: layer %d lacks the LayerNorm-fold column sums", li);
        c.XH = c.X;
        c.XL = reinterpret_cast<unsigned char*>(c.X) + (size_t)c.M * 768 * 2;
        c.stats = reinterpret_cast<float*>(c.ws + c.p.off_stats);
    }
    return 0;
}

// variable-length execution: compact the valid tokens, zero the padded positions of the result
static int setup_varlen(Ctx& c, float* eps_out) {
    const bg_denoiser_inputs* in = c.in;
    const int B = c.B;
    int* offs = reinterpret_cast<int*>(c.ws + c.p.off_rows);
    int* srow = reinterpret_cast<int*>(c.ws + c.p.off_rows + align_up((size_t)(B + 2 + P256_RULE_ENTRIES) * 4));
    const int n_mask = (c.net == BG_EDGEPOS) ? in->S : c.N, rep = (c.net == BG_EDGEPOS) ? c.E : 1;
    int rc;
    if (c.paired) {
        int* sd = reinterpret_cast<int*>(c.ws + c.p.off_slots);
        rc = compact_rows_paired(in->mask, B, n_mask, offs, srow, sd, sd + 2 * B, sd + 3 * B, c.s, offs + B + 2);
        c.slot_desc = sd;
    } else {
        rc = compact_rows(in->mask, B, n_mask, rep, offs, srow, c.s, offs + B + 2);
    }
    if (rc) return rc;
    c.offsets = offs; c.m_dev = offs + B; c.src_row = srow; c.rule = offs + B + 2;
    c.rows_hint = in->rows_hint > 0 ? in->rows_hint : 0.0;
    c.pairs_hint = in->pairs_hint > 0 ? in->pairs_hint : 0.0;
    c.rows_plan = in->rows_plan[0] > 0 ? in->rows_plan[0] : 0.0;
    // padded positions of the result are defined as 0 (the valid rows are scattered over this)
    const hipError_t he = hipMemsetAsync(eps_out, 0, (size_t)c.p.M * c.w->fc_out.n_out * sizeof(float), c.s);
    BG_REQUIRE(he == hipSuccess, (int)he, "bg_denoiser_fwd: hipMemsetAsync failed: %s", hipGetErrorString(he));
    return 0;
}

// time (+ class) embedding -> one vector per sample, c.cvec
static int cond_vectors(Ctx& c) {
    const bg_denoiser_weights* w = c.w;
    const bg_denoiser_inputs* in = c.in;
    const int nt = in->n_timesteps;
    // the time-embedding MLP is a function of the weights and the timestep only: looked up in the table the caller precomputed
    if (w->time_table != nullptr && w->time_table_rows > 0)
        return cond_vector_table(w->time_table, w->time_table_rows, in->timesteps, nt, w->class_embed, in->class_label, c.cvec, c.B, c.s);
    float* small = reinterpret_cast<float*>(c.ws + c.p.off_small);
    float* sc = small;                           // [nt,768] sincos
    float* temb = small + (size_t)3 * c.B * 768; // [nt,768]
    int rc;
    if ((rc = sincos_embed(in->timesteps, nt, sc, c.s))) return rc;
    if ((rc = embed_mlp(c, w->time_embed, sc, 768, nt, temb, 768))) return rc;
    return cond_vector(temb, nt, w->class_embed, in->class_label, c.cvec, c.B, c.s);
}

// token embeddings -> the stream X [M,768]
static int token_embeds(Ctx& c) {
    const bg_denoiser_weights* w = c.w;
    const bg_denoiser_inputs* in = c.in;
    const int net = c.net, M = c.M, N = c.N, E = c.E, F = c.p.F;
    int rc;
    // step-invariant part (per face): SurfZ: p_embed(surfPos); Edge nets: surfp_embed(surfPos)+surfz_embed(surfZ)
    float* fcond = nullptr;
    // SurfZNet, variable-length, no conditioning cache: p_embed(surfPos) is computed on the compact rows (the cache, when
    // the caller provides one, stays in the padded per-face layout so that it does not depend on the mask)
    const bool fcond_compact = c.varlen && net == BG_SURFZ && in->cond_cache == nullptr;
    if (net != BG_SURFPOS) {
        fcond = in->cond_cache ? in->cond_cache : reinterpret_cast<float*>(c.ws + c.p.off_f);
        if (!(in->cond_cache && in->cond_cache_valid)) {
            if (net == BG_SURFZ && fcond_compact) {
                // faces == tokens: without a cache to fill, only the valid faces need their conditioning embed
                if ((rc = embed_mlp(c, w->embed[1], in->surf_pos, 6, c.paired ? M : F, fcond, 768, {}, {}, TOK | GATHER))) return rc;
            } else if (net == BG_SURFZ) {
                if ((rc = embed_mlp(c, w->embed[1], in->surf_pos, 6, F, fcond, 768))) return rc;
            } else {
                if ((rc = embed_mlp(c, w->embed[0], in->surf_pos, 6, F, fcond, 768))) return rc;
                if ((rc = embed_mlp(c, w->embed[1], in->surf_z, 48, F, fcond, 768, Addend{fcond, 768, 1}))) return rc;
            }
        }
    }
    // (variable-length: rows are the compact tokens; x is gathered, cvec [B] and the per-face conditioning
    //  fcond [B*S] -- kept in the padded layout, so the conditioning cache is unaffected -- are looked up through the
    //  row map: sample = token / N, face = token / E)
    const Addend per_sample{c.cvec, 768, N}, stream{c.X, 768, 1};
    const unsigned tokens = TO_STREAM | TOK | GATHER;
    switch (net) {
        case BG_SURFPOS:   // tokens = p_embed(x) + c
            return embed_mlp(c, w->embed[0], in->x, 6, M, c.X, 768, per_sample, {}, TO_STREAM);
        case BG_SURFZ:     // tokens = z_embed(x) + p_embed(surfPos) + c
            return embed_mlp(c, w->embed[0], in->x, 48, M, c.X, 768, per_sample, Addend{fcond, 768, 1},
                             tokens | MAP_ADD | (fcond_compact ? 0 : MAP_ADD2));
        case BG_EDGEPOS:   // tokens = edgep_embed(x) + surf[m/E] + c
            return embed_mlp(c, w->embed[2], in->x, 6, M, c.X, 768, per_sample, Addend{fcond, 768, E}, tokens | MAP_ADD | MAP_ADD2);
        default:           // EdgeZ: edgez_embed(x[:, :12]) + vertp_fc(x[:, 12:]) + edgep_embed(edgePos) + surf[m/E] + c
            if ((rc = embed_mlp(c, w->embed[3], in->x, 18, M, c.X, 768, per_sample, Addend{fcond, 768, E}, tokens | MAP_ADD | MAP_ADD2))) return rc;
            if ((rc = embed_mlp(c, w->embed[4], in->x + 12, 18, M, c.X, 768, stream, {}, tokens))) return rc;
            return embed_mlp(c, w->embed[2], in->edge_pos, 6, M, c.X, 768, stream, {}, tokens);
    }
}

// key-padding mask [B,N] + the pre-LN encoder layers
static int encoder_layers(Ctx& c) {
    const bg_denoiser_weights* w = c.w;
    int rc;
    c.key_pad = c.varlen ? nullptr : c.in->mask;                  // (variable-length: every compact row is a valid key)
    if (c.net == BG_EDGEPOS && c.in->mask && !c.varlen) {
        uint8_t* mexp = c.ws + c.p.off_mask;
        const size_t n = (size_t)c.M;
        const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
        hipLaunchKernelGGL(expand_mask_kernel, dim3(grid), dim3(256), 0, c.s, c.in->mask, mexp, n, c.E);
        if ((rc = launch_status("expand_mask"))) return rc;
        c.key_pad = mexp;
    }
    BG_REQUIRE(!c.paired || c.fold, BG_E_ARG, "bg_denoiser_fwd: slot-packed execution needs the LayerNorm-fold operands");
    c.fused_qkv = c.fold && !c.varlen && g_tune[BG_TUNE_QKV_ATTN] != 1 &&
                  qkv_attn_eligible(c.B, c.N, c.dtype, c.stats, w->layers[0].qkv_colsum, w->layers[0].b_qkv) &&
                  (g_tune[BG_TUNE_QKV_ATTN] == 2 || qkv_attn_worthwhile(c.B, c.N));
    for (int li = 0; li < w->n_layer; ++li)
        if ((rc = c.fold ? encoder_layer_folded(c, w->layers[li]) : encoder_layer_unfolded(c, w->layers[li]))) return rc;
    return 0;
}

// final LayerNorm + fc_out -> eps_out (variable-length: the compact result rows are scattered into the zero-filled padded eps_out)
static int output_tail(Ctx& c, float* eps_out) {
    const bg_mlp_weights& mo = c.w->fc_out;
    const int M = c.M;
    int rc;
    if (mo.w0_colsum != nullptr) {
        BG_REQUIRE(c.fold && mo.w0_dtype == c.dtype && ln_silu_out_supported(mo.n_out, mo.n_out_pad), BG_E_ARG,
                   "bg_denoiser_fwd: fc_out carries the folded final LayerNorm (w0_colsum): needs the 16-bit LayerNorm-fold layers and n_out <= 48");
        // 16-bit modes: the final LayerNorm is folded into fc_out.0 (the epilogue of QKV / FFN1: raw XH rows in, the statistics the
        // last FFN2 left behind), and LayerNorm + SiLU + Linear(768, n_out) are one launch (out_tail.hip) -- two launches, and the
        // [M, 768] intermediate crosses HBM once, in 16 bits
        GemmArgs g0 = linear(c.XH, 768, mo.w0, mo.b0, c.H, 768, M, 768, 768, 768, c.dtype);
        ln_fold_in(g0, c.stats, mo.w0_colsum);
        token_rows(c, g0);
        if ((rc = gemm(g0, c.dtype, c.s))) return rc;
        return ln_silu_out(c.H, mo.ln_g, mo.ln_b, mo.w3, mo.b3, eps_out, mo.n_out, mo.n_out_pad, M, c.dtype, 1e-5f, c.s, c.m_dev,
                           c.varlen ? c.src_row : nullptr, c.rows_hint);
    }
    // fc_out.0 reads the final-LN output from H and writes its fp32 result to R; the LN+SiLU then overwrites H.
    if (c.fold) rc = layernorm768_split(c.XH, c.XL, c.w->lnf_g, c.w->lnf_b, c.H, c.dtype, M, 1e-5f, c.s, c.m_dev, c.rows_hint);
    else rc = layernorm768(c.X, c.w->lnf_g, c.w->lnf_b, c.H, c.dtype, M, 1e-5f, /*silu=*/0, c.s, c.m_dev, c.rows_hint);
    if (rc) return rc;
    return embed_mlp(c, mo, c.H, 768, M, eps_out, mo.n_out, {}, {}, TOK | SCATTER);
}

// concurrent: sibling sample groups of the same call are in flight on forked streams (tells the GEMM launcher that a partial
// round of tiles will be filled by the other group: bg_common.h p256_rows)
static int run(const bg_denoiser_weights* w, const bg_denoiser_inputs* in, float* eps_out, void* workspace,
               size_t ws_bytes, hipStream_t s, bool concurrent = false) {
    int rc;
    if ((rc = check_args(w, in, eps_out, workspace))) return rc;
    Ctx c;
    c.s = s;
    c.concurrent = concurrent ? 1 : 0;
    if ((rc = bind_workspace(c, w, in, workspace, ws_bytes))) return rc;
    if (c.varlen && (rc = setup_varlen(c, eps_out))) return rc;
    if ((rc = cond_vectors(c))) return rc;
    if ((rc = token_embeds(c))) return rc;
    if ((rc = encoder_layers(c))) return rc;
    return output_tail(c, eps_out);
}

}  // namespace bg

namespace bg {
constexpr int MAX_SPLIT = 4;
// contiguous sample groups of an n-way split (sizes differ by at most one)
static inline void split_range(int B, int n, int k, int& lo, int& hi) {
    const int base = B / n, rem = B % n;
    lo = k * base + (k < rem ? k : rem);
    hi = lo + base + (k < rem ? 1 : 0);
}
static size_t plan_total_split(int net, int B, int S, int E, int dtype, int n) {
    size_t t = 0;
    for (int k = 0; k < n; ++k) {
        int lo, hi;
        split_range(B, n, k, lo, hi);
        if (hi > lo) t += align_up(plan(net, hi - lo, S, E, dtype).total);
    }
    return t;
}
// helper streams + fork / join events of the split mode: created once PER DEVICE (a process that drives nets on several devices
// must not enqueue a sub-batch on another device's stream), used under a mutex (enqueue only: microseconds)
struct SplitState {
    hipStream_t aux[MAX_SPLIT - 1];
    hipEvent_t fork, join[MAX_SPLIT - 1];
    bool tried = false, ok = false;
};
constexpr int MAX_SPLIT_DEVICES = 64;
static SplitState g_split_dev[MAX_SPLIT_DEVICES];
static std::mutex g_split_mutex;
// (called with g_split_mutex held) -> the state of the CURRENT device, or nullptr
static SplitState* split_state() {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_SPLIT_DEVICES) return nullptr;
    SplitState& st = g_split_dev[dev];
    if (!st.tried) {
        st.tried = true;
        bool ok = hipEventCreateWithFlags(&st.fork, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; i < MAX_SPLIT - 1 && ok; ++i)
            ok = hipStreamCreateWithFlags(&st.aux[i], hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&st.join[i], hipEventDisableTiming) == hipSuccess;
        st.ok = ok;
    }
    return st.ok ? &st : nullptr;
}
}  // namespace bg

extern "C" int bg_slot_packing_applies(int net, int B, int S, int E, int dtype, int fold) {
    // the predicate bg_denoiser_fwd itself evaluates for a variable-length call (`paired`), for hosts that want to compute rows_plan
    if (net < BG_EDGEPOS) E = 1;
    return (bg::slot_packing_applies(net, B, S, E, dtype) && fold != 0 && bg::g_tune[BG_TUNE_QKV_ATTN] != 1) ? 1 : 0;
}

extern "C" size_t bg_workspace_bytes(int net, int B, int S, int E, int dtype) {
    if (B <= 0 || S <= 0) return 0;
    if (net < BG_EDGEPOS) E = 1;
    if (E <= 0) return 0;
    size_t t = bg::plan(net, B, S, E, dtype).total;
    for (int n = 2; n <= bg::MAX_SPLIT; ++n) {
        const size_t ts = bg::plan_total_split(net, B, S, E, dtype, n);
        t = ts > t ? ts : t;
    }
    return t;
}

extern "C" int bg_denoiser_fwd(const bg_denoiser_weights* w, const bg_denoiser_inputs* in, float* eps_out,
                               void* workspace, size_t workspace_bytes, bg_stream_t stream) {
    using namespace bg;
    BG_REQUIRE(w && in, BG_E_ARG, "bg_denoiser_fwd: null descriptor");
    hipStream_t s = (hipStream_t)stream;
    BG_REQUIRE(in->n_split >= 0, BG_E_ARG, "bg_denoiser_fwd: n_split must be >= 0 (got %d)", in->n_split);
    const int ns = in->n_split > MAX_SPLIT ? MAX_SPLIT : in->n_split;
    if (ns < 2 || in->B < ns) return run(w, in, eps_out, workspace, workspace_bytes, s);

    // ---- n-way split over sample groups, one stream each, fork / join by events on the caller's stream ----
    const int net = w->net;
    BG_REQUIRE(net >= BG_SURFPOS && net <= BG_EDGEZ, BG_E_ARG, "bg_denoiser_fwd: bad net id %d", net);
    BG_REQUIRE(in->B > 0 && in->S > 0 && eps_out && workspace, BG_E_ARG, "bg_denoiser_fwd: null pointer / empty shape");
    const int S = in->S, E = (net >= BG_EDGEPOS) ? in->E : 1;
    BG_REQUIRE(E > 0, BG_E_SHAPE, "bg_denoiser_fwd: empty shape");
    BG_REQUIRE(((uintptr_t)workspace & 255) == 0, BG_E_ALIGN, "bg_denoiser_fwd: workspace must be 256-byte aligned");
    BG_REQUIRE(workspace_bytes >= plan_total_split(net, in->B, S, E, w->dtype, ns), BG_E_WORKSPACE,
               "bg_denoiser_fwd: workspace too small for n_split = %d", ns);
    static const int kInCols[4] = {6, 48, 6, 18};                 // channels of x per net (SurfPos, SurfZ, EdgePos, EdgeZ)
    const size_t tok = (size_t)S * E;
    const size_t mask_per_sample = (net == BG_EDGEZ) ? tok : (size_t)S;
    std::lock_guard<std::mutex> lock(g_split_mutex);
    SplitState* sp = split_state();
    BG_REQUIRE(sp != nullptr, BG_E_ARG, "bg_denoiser_fwd: could not create the helper streams of the split mode on this device");
    SplitState& g_split = *sp;
    hipError_t he = hipEventRecord(g_split.fork, s);
    BG_REQUIRE(he == hipSuccess, (int)he, "bg_denoiser_fwd: hipEventRecord failed: %s", hipGetErrorString(he));
    unsigned char* wsp = reinterpret_cast<unsigned char*>(workspace);
    int rc = 0;
    for (int k = 0; k < ns; ++k) {
        int lo, hi;
        split_range(in->B, ns, k, lo, hi);
        bg_denoiser_inputs sub = *in;
        sub.B = hi - lo;
        sub.n_split = 1;
        sub.x = in->x + (size_t)lo * tok * kInCols[net];
        if (in->surf_pos) sub.surf_pos = in->surf_pos + (size_t)lo * S * 6;
        if (in->surf_z) sub.surf_z = in->surf_z + (size_t)lo * S * 48;
        if (in->edge_pos) sub.edge_pos = in->edge_pos + (size_t)lo * tok * 6;
        if (in->mask) sub.mask = in->mask + (size_t)lo * mask_per_sample;
        if (in->n_timesteps == in->B) { sub.timesteps = in->timesteps + lo; sub.n_timesteps = sub.B; }
        if (in->class_label) sub.class_label = in->class_label + lo;
        if (in->cond_cache) sub.cond_cache = in->cond_cache + (size_t)lo * S * 768;
        sub.rows_hint = in->rows_hint * sub.B / in->B;            // estimates: proportional share
        sub.pairs_hint = in->pairs_hint * sub.B / in->B;
        sub.rows_plan[0] = in->rows_plan[k];                      // (exact per group, or 0)
        const size_t bytes = align_up(plan(net, sub.B, S, E, w->dtype).total);
        hipStream_t sk = k == 0 ? s : g_split.aux[k - 1];
        if (k > 0 && (he = hipStreamWaitEvent(sk, g_split.fork, 0)) != hipSuccess) { rc = (int)he; break; }
        rc = run(w, &sub, eps_out + (size_t)lo * tok * w->fc_out.n_out, wsp, bytes, sk, /*concurrent=*/true);
        if (rc) break;
        wsp += bytes;
    }
    // join every helper stream back into the caller's stream -- also after an error, so nothing is left dangling
    for (int k = 1; k < ns; ++k) {
        if (hipEventRecord(g_split.join[k - 1], g_split.aux[k - 1]) == hipSuccess)
            (void)hipStreamWaitEvent(s, g_split.join[k - 1], 0);
    }
    return rc;
}

// ---- stand-alone pieces of the whole-net call (same code paths, caller-owned scratch) ---------------------------------
extern "C" size_t bg_embed_mlp_scratch_bytes(int rows, int dtype) {
    if (rows <= 0) return 0;
    const size_t es = (dtype == BG_F32) ? 4 : 2;
    return bg::align_up((size_t)rows * 768 * es) + bg::align_up((size_t)rows * 768 * 4);
}

extern "C" int bg_embed_mlp_fwd(const bg_mlp_weights* m, int dtype, const void* x, int lda, int rows, float* out, int ldc,
                                const float* add, int ld_add, int add_div, void* scratch, size_t scratch_bytes,
                                bg_stream_t stream) {
    using namespace bg;
    BG_REQUIRE(m && x && out && scratch, BG_E_ARG, "bg_embed_mlp_fwd: null pointer");
    BG_REQUIRE(dtype == BG_F32 || dtype == BG_BF16 || dtype == BG_F16, BG_E_DTYPE, "bg_embed_mlp_fwd: dtype %d", dtype);
    BG_REQUIRE(rows > 0 && lda >= m->k_in && ldc >= m->n_out, BG_E_SHAPE, "bg_embed_mlp_fwd: bad shape");
    BG_REQUIRE(scratch_bytes >= bg_embed_mlp_scratch_bytes(rows, dtype), BG_E_WORKSPACE, "bg_embed_mlp_fwd: scratch too small");
    BG_REQUIRE(((uintptr_t)scratch & 255) == 0, BG_E_ALIGN, "bg_embed_mlp_fwd: scratch must be 256-byte aligned");
    bg_denoiser_weights none{};
    Ctx c;
    c.w = &none; c.s = (hipStream_t)stream; c.dtype = dtype; c.ws = reinterpret_cast<unsigned char*>(scratch);
    c.X = nullptr;
    c.H = c.ws;
    c.R = c.ws + align_up((size_t)rows * 768 * ((dtype == BG_F32) ? 4 : 2));
    return embed_mlp(c, *m, x, lda, rows, out, ldc, Addend{add, ld_add, add_div});
}

extern "C" size_t bg_encoder_layer_scratch_bytes(int B, int N, int dtype) {
    if (B <= 0 || N <= 0) return 0;
    const size_t es = (dtype == BG_F32) ? 4 : 2, M = (size_t)B * N;
    return bg::align_up(M * 768 * es) + bg::align_up(M * 2304 * es);
}


// One pre-LN encoder layer (nn.TransformerEncoderLayer(norm_first=True), network.py:1076-1078) on an fp32 residual
// stream x [B*N, 768], in place -- the unfolded formulation: LayerNorm kernels + unfolded weights (qkv_colsum == NULL).
extern "C" int bg_encoder_layer_fwd(const bg_layer_weights* L, int dtype, float* x, const uint8_t* key_pad, int B, int N,
                                    void* scratch, size_t scratch_bytes, bg_stream_t stream) {
    using namespace bg;
    BG_REQUIRE(L && x && scratch, BG_E_ARG, "bg_encoder_layer_fwd: null pointer");
    BG_REQUIRE(dtype == BG_F32 || dtype == BG_BF16 || dtype == BG_F16, BG_E_DTYPE, "bg_encoder_layer_fwd: dtype %d", dtype);
    BG_REQUIRE(B > 0 && N > 0, BG_E_SHAPE, "bg_encoder_layer_fwd: empty shape");
    BG_REQUIRE(L->qkv_colsum == nullptr && L->w1_colsum == nullptr && L->ln1_g && L->ln2_g, BG_E_ARG,
               "bg_encoder_layer_fwd: takes unfolded weights (the LayerNorm-folded layers run inside bg_denoiser_fwd)");
    BG_REQUIRE(scratch_bytes >= bg_encoder_layer_scratch_bytes(B, N, dtype), BG_E_WORKSPACE, "bg_encoder_layer_fwd: scratch too small");
    BG_REQUIRE(((uintptr_t)scratch & 255) == 0, BG_E_ALIGN, "bg_encoder_layer_fwd: scratch must be 256-byte aligned");
    Ctx c;
    c.w = nullptr; c.s = (hipStream_t)stream; c.dtype = dtype; c.ws = reinterpret_cast<unsigned char*>(scratch);
    c.B = B; c.N = N; c.M = B * N; c.key_pad = key_pad;
    c.X = x;
    c.H = c.ws;
    c.R = c.ws + align_up((size_t)c.M * 768 * ((dtype == BG_F32) ? 4 : 2));
    return encoder_layer_unfolded(c, *L);
}
