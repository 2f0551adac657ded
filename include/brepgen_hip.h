/*
 * brepgen_hip.h -- C ABI of libbrepgen_hip.so (gfx950 / MI355X only).
 *
 * The reference (samxuxiang/BrepGen) has no FFI / plugin layer: its hot path is
 * Python calling torch ops.  This ABI is therefore the boundary a maintainer
 * would bind *under* the reference's Python call surface; every entry point
 * names the reference code it replaces (file:line in /root/reference).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. the PyTorch
 *     caching allocator), including the workspace; the library never allocates,
 *     never synchronises, keeps no global state; everything is enqueued on the
 *     `stream` argument (pass torch.cuda.current_stream().cuda_stream);
 *   - tensors are dense row-major, batch-first: tokens [B, N, C] == rows [M=B*N, C];
 *   - return 0 on success, a positive hipError_t from the launch, or a negative
 *     BG_E_* argument error; bg_last_error() gives the thread-local message;
 *   - nothing throws across the boundary.
 */
#ifndef BREPGEN_HIP_H
#define BREPGEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BG_ABI_VERSION 7

typedef void* bg_stream_t;              /* hipStream_t */

enum bg_dtype { BG_F32 = 0, BG_F16 = 1, BG_BF16 = 2 };
enum bg_act { BG_ACT_NONE = 0, BG_ACT_RELU = 1 };
enum bg_net { BG_SURFPOS = 0, BG_SURFZ = 1, BG_EDGEPOS = 2, BG_EDGEZ = 3 };
enum bg_err { BG_E_ARG = -1, BG_E_SHAPE = -2, BG_E_WORKSPACE = -3, BG_E_DTYPE = -4, BG_E_ALIGN = -5 };

#define BG_D_MODEL 768
#define BG_N_HEAD 12
#define BG_D_HEAD 64
#define BG_D_FF 1024
#define BG_MAX_LAYERS 12
#define BG_MAX_EMBEDS 5

int bg_abi_version(void);
const char* bg_last_error(void);

/* ---- elementwise / normalisation ------------------------------------------------------ */

/* network.py:1043-1063 sincos_embedding: out[i, 0:384]=cos(t_i*f), out[i,384:768]=sin(t_i*f). */
int bg_sincos_embed(const int64_t* timesteps, int n, float* out /*[n,768]*/, bg_stream_t stream);

/* torch.nn.LayerNorm(768, eps) as used at network.py:1076-1099 (optionally followed by SiLU, the
 * `LayerNorm -> SiLU` pair inside every embed MLP).  x fp32 [M,768]; y fp32 or bf16 [M,768]. */
int bg_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y, int y_dtype,
                     int M, float eps, int fuse_silu, bg_stream_t stream);

/* nn.Linear (+ReLU) (+residual / broadcast add) -- every addmm of network.py:1076-1099.
 *   out[m,n] = act(sum_k a[m,k]*w[n,k] + bias[n]) + (add ? add[(m/add_div)*ld_add + n] : 0)
 * a: [M,K] dtype ab_dtype (BG_F32 or BG_BF16), row stride lda; w: [N_pad,K] same dtype (nn.Linear
 * layout, row stride K); out: fp32 or bf16, row stride ldc, only columns < N are written.
 * BG_BF16: K % 64 == 0, N_pad % 64 == 0 (weights zero-padded by the packer).  BG_F32: any shape.
 * `add` may alias `out` (in-place residual, add_div = 1). */
int bg_gemm_bias_act_fwd(const void* a, int lda, const void* w, const float* bias, void* out, int ldc,
                         int M, int N, int N_pad, int K, int ab_dtype, int out_dtype, int act,
                         const float* add, int ld_add, int add_div, bg_stream_t stream);

/* The same GEMM with every epilogue option of the 16-bit kernels, as one descriptor.  Beyond bg_gemm_bias_act_fwd:
 *   add2            second fp32 addend, row (m / add2_div)
 *   out_lo          split output: the fp32 result v is stored as hi = T(v) -> out and lo = T(v - hi) -> out_lo
 *                   (two 16-bit planes, row stride ldc); hi is directly the next GEMM's A operand
 *   res_hi, res_lo  split residual addend rows [M,N] (row stride ld_res); may alias out / out_lo (in place)
 *   stats_out       [N_pad/64][M][2] fp32 (part-major): per 64-column group (sum, sum of squares) of v
 *   stats_in, colsum  LayerNorm fold: a holds raw (un-normalised) 16-bit rows, w = T(gamma * W), bias = b + W beta,
 *                   colsum[n] = sum_k w[n,k]; the epilogue computes act(rstd_m * acc - mean_m * rstd_m * colsum[n] +
 *                   bias[n]) with mean / rstd summed from stats_in [K/64][M][2] (written by a producer's stats_out).
 *                   (Launches large enough for the 256 x 256 persistent kernel take it when M is even and stats_in is
 *                   16-byte aligned -- it fetches the partials with its LDS-DMA stream, two rows per element; otherwise the
 *                   128 x 128 kernel runs.  Same bits either way.)
 * The new options need ab_dtype BG_BF16 | BG_F16, N == N_pad and ldc % 8 == 0. */
typedef struct {
    const void* a; int lda;
    const void* w; const float* bias;
    void* out; int ldc;
    int M, N, N_pad, K;
    int ab_dtype, out_dtype, act;
    const float* add; int ld_add, add_div;
    const float* add2; int ld_add2, add2_div;
    void* out_lo;
    const void* res_hi; const void* res_lo; int ld_res;
    float* stats_out;
    const float* stats_in; const float* colsum; float ln_eps;
} bg_gemm_desc;
int bg_gemm_ex_fwd(const bg_gemm_desc* d, bg_stream_t stream);

/* Convolution as an IMPLICIT GEMM (the 3x3 / k5 convolutions of the VAE decoders: ResnetBlock2D.conv1/conv2, Upsample2D.conv,
 * ResConvBlock.conv_1/conv_2 -- network.py:30-83, 188-299, 948-1040 via diffusers): the MFMA GEMM's activation loader
 * gathers the window straight from the channels-last tensor, so the kh*kw-fold im2col matrix is never written.
 *   x     16-bit channels-last activations [S, H, W, C] (1-D: H = 1), ALREADY normalised / activated (bg_im2col with a 1x1
 *         window does GroupNorm + SiLU/GELU + the cast in one pass); C % 64 == 0, C / 64 a power of two
 *   'same' convolution, stride 1, window kh x kw (odd), on the nearest-upsampled grid (H << up, W << up) = (Ho, Wo), both
 *         powers of two; zero padding outside (padded taps read zero_page: one pixel = 2 * C bytes of zeros on the device)
 *   w     [N, kh*kw*C] 16-bit, tap-major (tap = ky*kw + kx, then channel), N % 128 == 0;  bias fp32 [N] or NULL
 *         -- or a NARROW output, N < 128 (the decoders' conv_out, network.py:786-858 / 948-1040: 3 channels): w [128, kh*kw*C] and
 *         bias [128] zero-padded by the caller, no residual; one 128-column tile per row panel, only the N real columns stored
 *   out   fp32 [S*Ho*Wo, N] (row stride ldc >= N) = conv + bias (+ add: fp32 residual rows, row stride ld_add)
 * Needs at least 64 output tiles of 128 x 128 (it runs on the persistent kernel); smaller problems: im2col + GEMM. */
typedef struct {
    const void* x; int S, H, W, C;
    int kh, kw, up;
    const void* w; const float* bias; int N;
    float* out; int ldc;
    const float* add; int ld_add;
    int dtype;                 /* BG_BF16 | BG_F16: operand dtype of x and w */
    const void* zero_page;
} bg_conv_desc;
int bg_conv_gemm_fwd(const bg_conv_desc* d, bg_stream_t stream);

/* LayerNorm(768) of rows given as the split pair x = hi + lo (two 16-bit planes of dtype `dtype`) -> y (same dtype):
 * the denoisers' final net.norm when the residual stream is kept split. */
int bg_layernorm_split_fwd(const void* hi, const void* lo, const float* gamma, const float* beta, void* y, int dtype,
                           int M, float eps, bg_stream_t stream);

/* First half of an input-embedding MLP, fused: out = SiLU(LayerNorm(x W0^T + b0)), x fp32 [rows, lda] (k in {6,12,48}
 * leading columns used), exact-fp32 matrix-core arithmetic, out [rows,768] fp32 / bf16 / fp16 (sub-keys .0 .1 + SiLU
 * of p_embed, z_embed, surfp_embed, surfz_embed, edgep_embed, edgez_embed, vertp_fc: network.py:1080-1085 etc.).
 * w0_mfma: see bg_mlp_weights. */
int bg_embed_ln_silu_fwd(const float* x, int lda, int rows, int k, const float* w0_mfma, const float* b0,
                         const float* ln_g, const float* ln_b, void* out, int out_dtype, float eps, bg_stream_t stream);

/* F.scaled_dot_product_attention inside nn.MultiheadAttention (network.py:1076-1078 via
 * torch/nn/modules/transformer.py slow path): qkv packed [B*N, 2304] (q|k|v, head h at columns
 * 64h..64h+63 of each third; q already multiplied by 1/8), key_pad uint8 [B,N] (1 = padded key, -inf)
 * or NULL; out [B*N,768].  dtype BG_BF16 or BG_F32.  A sample whose keys are all padded yields 0
 * (the reference yields NaN there; the pipeline never produces such a sample, sample.py:163,261). */
int bg_attn_fwd(const void* qkv, const uint8_t* key_pad, void* out, int B, int N, int dtype,
                bg_stream_t stream);
/* The same over a COMPACTED batch (variable-length execution): offsets int32 [B+1] on the device, sample b owns rows
 * offsets[b] .. offsets[b+1]-1 of qkv / out (at most N of them, every one a valid key; key_pad must then be NULL).
 * offsets == NULL is bg_attn_fwd.  Every kernel takes its rows from offsets[b] .. offsets[b+1]-1 alone: rows at and beyond offsets[B]
 * (qkv / out are usually sized for the bound B * N) are neither read nor written -- out keeps whatever it held there -- and a sample
 * with offsets[b] == offsets[b+1] costs nothing. */
int bg_attn_varlen_fwd(const void* qkv, const uint8_t* key_pad, void* out, int B, int N, int dtype,
                       const int* offsets, bg_stream_t stream);

/* ---- the attention core for TRAINING (csrc/attn_train.hip): forward that keeps the row log-sum-exp, dropout on the probabilities
 * (nn.MultiheadAttention(dropout=0.1) in net.train(), network.py:1076-1078), and the backward.  Layout as bg_attn_fwd: qkv
 * [B*N, 2304], key_pad uint8 [B, N] (1 = padded key) or NULL, out [B*N, 768]; dtype BG_BF16 / BG_F16 (MFMA, fp32 accumulation) or
 * BG_F32 (VALU restatement, sums accumulated in fp64).  The score is S = scale * q.k^T: q is NOT pre-scaled here.  N >= 1; B == 0 returns 0 without a
 * launch.  Nothing is allocated, no atomics: every output element has one writer and a fixed summation order, so two calls give the
 * same bits and a sample's results depend on that sample's rows alone.
 *
 * The dropout mask M is a pure function of (seed, draw_id, GLOBAL sample index g = first_sample + b, head, query, key): one
 * Philox4x32-10 block, key = seed, counter = (query << 16 | kb, low 32 bits of g, draw_id, 0xAD700000 | head << 12 | bits 32..43 of g),
 * gives the four words of keys 4 kb .. 4 kb + 3; a key is KEPT iff its word >= floor(dropout_p * 2^32) (formed in double), and kept
 * probabilities are multiplied by float(1 / (1 - dropout_p)).  0 <= dropout_p < 1; dropout_p == 0 runs kernels compiled without the
 * generator.  With dropout_p > 0, N <= 65536. */

/* Forward.  Reads qkv rows 0 .. B*N-1 and key_pad.  Writes out [B*N, 768] = (softmax(S) o M / (1 - p)) V and lse fp32 [B, 12, N] =
 * row maximum + log of the row sum of exp, taken BEFORE dropout (the softmax normaliser does not see the mask, as in torch).  A
 * sample whose keys are all padded gives out = 0 and lse = 0. */
int bg_attn_train_fwd(const void* qkv, const uint8_t* key_pad, void* out, float* lse, int B, int N, int dtype, float scale,
                      double dropout_p, unsigned long long seed, unsigned draw_id, long long first_sample, bg_stream_t stream);
/* Scratch of bg_attn_bwd, rounded up to 256 bytes: delta [B, 12, N] fp32; BG_F32: followed by the row maximum and the row sum of
 * exp, [B, 12, N] each (the fp32 kernels normalise as torch does, P = exp(S - max) / sum, and do not read lse: rounded to fp32 it would
 * cost several ulp in every P of a row).  0 for arguments bg_attn_bwd rejects. */
size_t bg_attn_bwd_workspace_bytes(int B, int N, int dtype);
/* Backward.  Reads qkv and key_pad, lse as bg_attn_train_fwd left it, dout [B*N, 768] (dtype of qkv) and the same dropout key; the
 * forward's out is not needed.  Writes dqkv [B*N, 2304] (dq | dk | dv, dtype of qkv), EVERY element, rows of padded tokens included
 * (nobody has to zero it first), and the workspace as bg_attn_bwd_workspace_bytes lays it out.  P = exp(S - lse) recomputed in fp32;
 * dV = (P o M/(1-p))^T dO;  dP = (dO V^T) o M/(1-p);  delta_i = sum_j P_ij dP_ij (= sum_d dO_id O_id, summed as torch's softmax
 * backward sums it);  dS = P o (dP - delta);  dQ = scale dS K;  dK = scale dS^T Q.  Padded keys have P = 0 exactly: their dK and
 * dV rows are exactly 0, and an all-padded sample's gradients are all 0.  A non-finite dout makes delta, dP and dS of its sample
 * non-finite: that sample's gradients contain inf / NaN (a GradScaler's found_inf trips), the other samples' stay finite.
 * General path, any N, two launches: dQ (a workgroup owns 128 queries of one (sample, head) and walks the keys twice: delta, then dS
 * and dQ); dK / dV (a workgroup owns 128 keys and walks the queries).  Short path, N <= 64 and 16-bit operands, ONE launch with
 * nothing recomputed: a workgroup holds one (sample, head), P~ and dS cross the LDS once; its dQ is the general path's bit for bit,
 * its dK / dV sum the queries in another order.  variant picks: BG_ATTN_BWD_AUTO (the short path where it applies),
 * BG_ATTN_BWD_GENERAL, BG_ATTN_BWD_SHORT (BG_E_SHAPE where it does not apply).  first_sample + B <= 2^44. */
enum bg_attn_bwd_variant { BG_ATTN_BWD_AUTO = 0, BG_ATTN_BWD_GENERAL = 1, BG_ATTN_BWD_SHORT = 2 };
int bg_attn_bwd(const void* qkv, const uint8_t* key_pad, const float* lse, const void* dout, void* dqkv, int B, int N,
                int dtype, float scale, double dropout_p, unsigned long long seed, unsigned draw_id, long long first_sample,
                int variant, void* workspace, size_t workspace_bytes, bg_stream_t stream);
/* The keep mask itself, uint8 [B, 12, N, N] (1 = kept), from the same key: the replay / test entry (a host can reproduce a run's
 * masks from it, or from the counter layout above).  Writes every element; reads nothing.  N <= 65536. */
int bg_attn_dropout_mask(uint8_t* mask, int B, int N, double dropout_p, unsigned long long seed, unsigned draw_id, long long first_sample,
                         bg_stream_t stream);

/* ---- the Linear layers' backward (csrc/linear_bwd.hip): what torch's autograd does for the four nn.Linear of an encoder layer
 * (network.py:1076-1078) under autocast.  y = x W^T + b and dX = dY W run on bg_gemm_ex_fwd (dX: a = dY, w = W^T as bg_weight_cast
 * writes it); the weight and bias gradients are the product below. */

/* dw [N, K] (nn.Linear layout) = sum_m dy[m, n] x[m, k] and db [N] = sum_m dy[m, n] (db may be NULL) in ONE launch (two with a
 * split).  dy [M, N] and x [M, K] are 16-bit of `dtype` (BG_BF16 | BG_F16), row-major with row strides ld_dy >= N, ld_x >= K in
 * elements, multiples of 8; all bases 16-byte aligned.  out_dtype: BG_F32 (fp32 master parameters: the fp32 sum is never rounded to
 * 16 bits) or `dtype`.  N % 128 == 0 and K % 128 == 0, else BG_E_SHAPE; M >= 1; M == 0 writes zeros to dw / db.  Only rows < M and
 * columns < N (K) of dy (x) are read.
 * A workgroup owns one 128 x 128 tile of dw and one contiguous slice of the M rows, walked in steps of 32 rows; slice s of S covers
 * rows [s R, min(M, (s + 1) R)), R = 32 * ceil(ceil(M / 32) / S).  split = S: 0 = auto (bg_linear_wgrad_split), or 1 .. 64; an S that
 * leaves a slice empty is BG_E_ARG.  S == 1 writes dw / db directly and needs no workspace (NULL is fine); S > 1 writes fp32 partials
 * [S][N][K] then [S][N] to the workspace and a second kernel adds them in index order.  A workspace smaller than
 * bg_linear_wgrad_workspace_bytes is BG_E_ARG.  No atomics, one writer per element, fixed summation order: two calls give the same
 * bits, and with fp32 output row n of dw depends on column n of dy alone.  A non-finite dy[m, n] makes dw[n, :] and db[n] non-finite
 * (a GradScaler's found_inf trips) and leaves the other rows finite. */
int bg_linear_wgrad(const void* dy, int ld_dy, const void* x, int ld_x, void* dw, void* db, int M, int N, int K, int dtype,
                    int out_dtype, int split, void* workspace, size_t workspace_bytes, bg_stream_t stream);
/* 0 for split == 1 (or an auto split that resolves to 1), else 4 * S * N * (K + 1) rounded up to 256 bytes; 0 for rejected arguments. */
size_t bg_linear_wgrad_workspace_bytes(int M, int N, int K, int split);
/* host-side plan, no device call: the S that split = 0 resolves to (1 for rejected arguments) */
int bg_linear_wgrad_split(int M, int N, int K);
/* src [R, C] (fp32, or 16-bit of `dtype`) -> dst [R, C] and / or dst_t [C, R], both 16-bit of `dtype` (BG_BF16 | BG_F16, round to
 * nearest even): autocast's per-call weight cast, and the W^T the data-gradient GEMM takes as its w.  Either output may be NULL, not
 * both.  R % 64 == 0, C % 64 == 0; dense, 16-byte aligned.  One launch: 64 x 64 tiles transposed through LDS. */
int bg_weight_cast(const void* src, int src_dtype, int R, int C, void* dst, void* dst_t, int dtype, bg_stream_t stream);

/* ---- the glue of an encoder layer in TRAINING (csrc/layer_train.hip): what nn.TransformerEncoderLayer(768, 12, 1024, dropout,
 * norm_first=True) in net.train() does between the attention core and the Linear products above -- LayerNorm forward and backward,
 * dropout + residual add, ReLU + dropout.  Rows are dense, [M, C] row-major, all bases 16-byte aligned (stats: 8).  Nothing is
 * allocated, no atomics: every output element has one writer and a fixed summation order, so two calls give the same bits.  M == 0
 * returns 0 without a launch (bg_ln_bwd: see there).  16-bit data moves 16 bytes per lane; grids are capped at 2048 workgroups and
 * stride over the rest.
 *
 * LayerNorm over 768 columns.  x is the residual stream, BG_F32 / BG_F16 / BG_BF16; y (and dy) is in y_dtype: any of the three for
 * an fp32 x, x's own dtype or BG_F32 for a 16-bit x (BG_E_DTYPE otherwise).  gamma / beta fp32 [768].  A half-wave of 32 lanes owns a
 * row; lane l holds the 8-column chunks l, l + 32, l + 64.  Every row sum adds a chunk's 8 values pairwise, the lane's three chunks in
 * order, then the 32 lanes by a butterfly (offsets 16, 8, 4, 2, 1). */

/* y = (x - mean) * rstd * gamma + beta, rounded ONCE from the fp32 result to y_dtype (autocast's fp32 LayerNorm plus the cast that
 * follows it, in one pass), and stats fp32 [M, 2] = (mean, rstd) per row.  Two passes over the row held in registers: mean = sum / 768,
 * then var = (sum of (x - mean)^2) / 768, rstd = 1 / sqrtf(var + eps) -- rows with |mean| >> std keep their variance, a constant row
 * has var = 0 exactly and y = beta. */
int bg_ln_train_fwd(const void* x, int x_dtype, const float* gamma, const float* beta, void* y, int y_dtype, float* stats, int M,
                    float eps, bg_stream_t stream);
/* Workspace of bg_ln_bwd when dgamma / dbeta are asked for: G * 1536 doubles, G = min(ceil(M / (8 R)), 2048) workgroups,
 * R = min(max(ceil(M / 8192), 4), 64) rows per fp32 chain.  0 for M <= 0. */
size_t bg_ln_bwd_workspace_bytes(int M);
/* Reads dy [M, 768] (y_dtype), x and stats as bg_ln_train_fwd left them, gamma, and dskip [M, 768] (x_dtype; may be NULL): the
 * gradient that arrives over the residual connection, added in the same pass.  Writes dx [M, 768] in x_dtype, every element:
 *     xhat = (x - mean) * rstd;  g = gamma * dy;  dx = rstd * ((g - mean_c(g)) - xhat * mean_c(g * xhat)) + dskip
 * (mean_c: the row sum above / 768; `+ dskip` is `+ 0.0f` for a NULL dskip, so a zero dskip and none give the same bits).
 * dgamma [768] = sum_m dy * xhat and dbeta [768] = sum_m dy, fp32; both NULL = not computed (no workspace needed), one NULL is
 * BG_E_ARG.  Summation order: workgroup w takes the row chunks w, w + G, ...; in chunk c half-wave s adds rows c * 8 R + 8 i + s,
 * i = 0 .. R - 1, into an fp32 chain per column; the eight chains of a chunk are added in order of s, in fp64, into the workgroup's
 * fp64 sum, which goes to workspace[w][1536] (dgamma | dbeta); a second kernel adds the G partials of a column in fp64: 32
 * contiguous groups of ceil(G / 32) in index order, then the 32 group sums in order, rounded once to fp32.  A workspace smaller than
 * bg_ln_bwd_workspace_bytes(M) is BG_E_ARG; nothing beyond that size is written.  M == 0 with non-NULL dgamma / dbeta writes zeros.
 * A row of dx depends on its own row alone and a column of dgamma / dbeta on its own column alone: a non-finite dy[m, c] makes
 * dx[m, :], dgamma[c] and dbeta[c] non-finite (a GradScaler's found_inf trips) and nothing else. */
int bg_ln_bwd(const void* dy, int y_dtype, const void* x, int x_dtype, const float* stats, const float* gamma, const void* dskip,
              void* dx, float* dgamma, float* dbeta, int M, void* workspace, size_t workspace_bytes, bg_stream_t stream);

/* Elementwise dropout.  Rows are sequence-first: row r of [M, C] is token n = r / B of sample b = r % B (M % B == 0), global sample
 * g = first_sample + b.  The keep mask is a pure function of (seed, draw_id, site, n, g, column): one Philox4x32-10 block, key = seed,
 * counter = (n * (C / 8) + column_block, low 32 bits of g, draw_id, 0xD4090000 | site << 12 | bits 32..43 of g), serves the 8 columns
 * 8 column_block .. 8 column_block + 7; element j uses half-word j & 1 (low half first) of word j >> 1 and is KEPT iff that half-word
 * >= floor(p * 65536) (formed in double); kept values are multiplied by rp = float(1 / (1 - p)).  site 0 .. 3 tells the dropouts of a
 * layer apart (1 = dropout1, 2 = the FFN dropout, 3 = dropout2).  C % 8 == 0, M * C / 8 < 2^32, 0 <= p < 1,
 * first_sample + B <= 2^44.  A rank that owns samples [lo, hi) of a sharded batch passes first_sample = lo, B = hi - lo and gets its
 * rows of the single-GPU mask.  floor(p * 65536) == 0 (p == 0 in particular) runs kernels compiled without the generator. */

/* out = skip + keep * rp * branch.  branch is 16-bit (branch_dtype); skip and out are in stream_dtype = BG_F32 or branch_dtype.
 * Kept: float(skip) + float(branch) * rp in fp32, rounded once; dropped: skip's value.  out may be skip (in place). */
int bg_dropout_add_fwd(const void* branch, int branch_dtype, const void* skip, void* out, int stream_dtype, int M, int C, int B,
                       double p, unsigned long long seed, unsigned draw_id, int site, long long first_sample, bg_stream_t stream);
/* dbranch (branch_dtype) = keep ? float(dout) * rp : 0, from the same key; dout is in stream_dtype.  (The gradient of skip is dout.) */
int bg_dropout_bwd(const void* dout, int stream_dtype, void* dbranch, int branch_dtype, int M, int C, int B, double p,
                   unsigned long long seed, unsigned draw_id, int site, long long first_sample, bg_stream_t stream);
/* h = (keep && x > 0) ? round(float(x) * rp) : 0, x and h 16-bit of `dtype`.  rp >= 1: a kept positive x never rounds to 0, so h > 0
 * marks exactly the elements whose gradient passes.  A NaN in a kept element propagates; a DROPPED element is 0 whatever x holds
 * (torch's relu-then-dropout writes NaN * 0 = NaN there). */
int bg_relu_dropout_fwd(const void* x, void* h, int dtype, int M, int C, int B, double p, unsigned long long seed, unsigned draw_id,
                        int site, long long first_sample, bg_stream_t stream);
/* dx = (h > 0) ? round(float(dh) * rp) : 0 from the saved h: no mask is regenerated, no key is needed. */
int bg_relu_dropout_bwd(const void* h, const void* dh, void* dx, int dtype, int M, int C, double p, bg_stream_t stream);
/* The keep mask itself, uint8 [M, C] (1 = kept; 8-byte aligned): the replay / test entry.  Writes every element; reads nothing. */
int bg_dropout_mask(uint8_t* mask, int M, int C, int B, double p, unsigned long long seed, unsigned draw_id, int site,
                    long long first_sample, bg_stream_t stream);

/* ---- the denoisers' MLPs and loss in TRAINING (csrc/mlp_train.hip): nn.Sequential(Linear(k, 768), LayerNorm, SiLU, Linear(768, n))
 * with a THIN side -- the data embeds' k = 6 / 12 / 48 and fc_out's n = 6 / 18 / 48 (network.py:1076-1099) -- and the gradient of
 * the masked MSE.  The thin dimension s (n) is 1 .. 48, BG_E_SHAPE otherwise; the wide one is 768.  The [M, 768] operands are dense
 * and 16-byte aligned; the thin operands are read element by element, so they need element alignment only and may be strided.  Nothing
 * is allocated, no atomics, one writer per output element, every sum in the order stated: two calls give the same bits.  M == 0 returns
 * 0 without a launch (bg_thin_wgrad: zeros).  fma(a, b, c) below is the fused multiply-add, one rounding. */

/* y [M, 768] (y_dtype: any of the three) = x [M, s] W + b.  x: x_dtype (any of the three), row stride ldx >= s in elements -- a column
 * slice of wider rows is read in place, its other columns never.  W fp32: w_k_major == 0 takes it as [768, s] (an embed's first
 * nn.Linear weight), w_k_major != 0 as [s, 768] (fc_out's last weight, for its data gradient dA = dY W).  b fp32 [768] or NULL (= 0).
 * Order: acc = b[c]; acc = fma(x[m, k], W(k, c), acc) for k = 0 .. s - 1; rounded once to y_dtype. */
int bg_thin_expand(const void* x, int x_dtype, int ldx, const float* w, int w_k_major, const float* b, void* y, int y_dtype, int M,
                   int s, bg_stream_t stream);
/* y fp32 [M, n] dense = a [M, 768] W^T + b: fc_out's last Linear.  a 16-bit (a_dtype), W fp32 [n, 768] read as it is (no 16-bit
 * copy: the product keeps fp32 weights), b fp32 [n] or NULL.  Order: a half-wave owns a row, lane l the columns 8 (l + 32 j) + e;
 * p = 0; p = fma(a[m, c], W[i, c], p) over j = 0, 1, 2 and e = 0 .. 7 in that order; the 32 lanes by a butterfly (offsets 16, 8, 4,
 * 2, 1); + b[i] last. */
int bg_thin_contract(const void* a, int a_dtype, const float* w, const float* b, float* y, int M, int n, bg_stream_t stream);
/* G * (s8 * 768 + 768 + s8) doubles, s8 = 8 ceil(s / 8), for the plan below; 0 for M <= 0 or s outside 1 .. 48. */
size_t bg_thin_wgrad_workspace_bytes(int M, int s);
/* g fp32 = t^T u: t [M, s] (t_dtype: any of the three, row stride ldt >= s), u [M, 768] 16-bit dense.  g is [s, 768], or [768, s]
 * with g_transposed != 0 (an embed's dW0 = dH^T X in nn.Linear's layout).  colsum_of: 0 none (colsum NULL), 1 colsum [768] = column
 * sums of u (db0), 2 colsum [s] = column sums of t (db3), from the same launch.  Plan, a pure function of (M, s): cap = 256 / ceil(s
 * / 8) row workgroups at most, R = min(max(ceil(M / (8 cap)), 4), 64) rows per fp32 chain, chunks of 8 R rows, W = min(chunks, cap)
 * row workgroups; a workgroup (w, 256-column slab, group of 8 k) takes the chunks w, w + W, ...; in chunk c half-wave h walks the rows
 * c 8 R + 8 i + h, i = 0 .. R - 1, with acc = fma(t[m, k], u[m, c], acc) per (k, column); the eight chains of a chunk are added in order of h in fp64 into the
 * workgroup's fp64 sum (a column sum: fp32 chains acc += value of 8 rows, i = 8 j .. 8 j + 7, folded in order into the half-wave's
 * fp64 sum, then the eight half-waves in order of h), which goes to the workspace; a second kernel adds
 * the W partials in index order in fp64 and rounds once.  A workspace smaller than bg_thin_wgrad_workspace_bytes is BG_E_ARG.  A
 * non-finite u[m, c] reaches column c of g alone, a non-finite t[m, k] row k alone. */
int bg_thin_wgrad(const void* t, int t_dtype, int ldt, const void* u, int u_dtype, float* g, int g_transposed, float* colsum,
                  int colsum_of, int M, int s, void* workspace, size_t workspace_bytes, bg_stream_t stream);
/* h = SiLU(LayerNorm(x)) over 768 columns in one pass, SiLU(v) = v / (1 + expf(-v)) in fp32, and stats as bg_ln_train_fwd writes
 * them: the same row kernel (csrc/ln_rows.h), dtype pairs, layout and checks. */
int bg_ln_silu_train_fwd(const void* x, int x_dtype, const float* gamma, const float* beta, void* h, int h_dtype, float* stats, int M,
                         float eps, bg_stream_t stream);
/* = bg_ln_bwd_workspace_bytes(M) */
size_t bg_ln_silu_bwd_workspace_bytes(int M);
/* The backward of the above: v = xhat * gamma + beta recomputed from x and stats as the forward formed it, sg = 1 / (1 + expf(-v)),
 * dv = dh * (sg + v * sg * (1 - sg)), then bg_ln_bwd's pass with dv in dy's place (no dskip): dx, and dgamma / dbeta through the
 * same chains, workspace and fp64 merge. */
int bg_ln_silu_bwd(const void* dh, int h_dtype, const void* x, int x_dtype, const float* stats, const float* gamma, const float* beta,
                   void* dx, float* dgamma, float* dbeta, int M, void* workspace, size_t workspace_bytes, bg_stream_t stream);
/* The gradient of bg_masked_mse's mean: dpred fp32 [rows, ld], every element written --
 *     (pred - target) * coef,  coef = (2 * g[0]) / (out3[2] * (float)ncols)  in fp32
 * in columns [col0, col0 + ncols) of rows with row_mask == 0, exactly 0 elsewhere (a select: NaN / Inf there is not read).  out3:
 * bg_masked_mse's output of the same call (out3[2] = valid rows, read on the device); g: the upstream gradient, a device scalar (it
 * carries a GradScaler's scale).  No valid row: all zeros.  One launch, nothing is read back. */
int bg_masked_mse_bwd(const float* pred, const float* target, const uint8_t* row_mask, long long rows, int ld, int col0, int ncols,
                      const float* out3, const float* g, float* dpred, bg_stream_t stream);

/* ---- a VAE ResnetBlock2D's convolution layer in TRAINING (csrc/conv_train.hip): the backward of
 *     y = conv(act(GroupNorm(x))) + bias          (diffusers ResnetBlock2D.norm1/conv1, norm2/conv2 -- network.py via diffusers)
 * whose forward is bg_groupnorm_stats, bg_im2col with a 1x1 window (norm + activation + cast -> the 16-bit `a`) and bg_conv_gemm_fwd or
 * bg_im2col + bg_gemm_bias_act_fwd (see "VAE steps" below).  Activations are channels-last [S, H, W, C] (1-D: H = 1); convolutions are
 * stride 1 with 'same' zero padding, window kh x kw, both odd and <= 5; H and W are powers of two; 16-bit operands are BG_BF16 | BG_F16.
 * No atomics, one writer per output element, fixed summation order: two calls give the same bits.  Arguments are checked before any
 * launch.  The DATA gradient has no entry of its own: it is the 'same' forward convolution of dy (cast to 16 bits by bg_im2col with a
 * 1x1 window and no norm) with the data-gradient pack of bg_conv_weight_pack, on bg_conv_gemm_fwd or, below that entry's 64-tile
 * rule, bg_im2col + bg_gemm_bias_act_fwd.  The stride-2 (Downsample2D) and up-sampling (Upsample2D) convolutions: "resampling
 * convolutions in TRAINING" below.  Not covered: conv_in / conv_out (3 and 6 channels), the mid-block attention, the 1-D ResConvBlock and
 * cubic resamplers, the posterior's backward. */

/* dw [N, kh*kw*C] (tap-major / channel-minor: tap = ky*kw + kx, the layout of the forward's packed weight) and db [N] (may be NULL):
 *     dw[n, tap, c] = sum_{s,y,x} dy[s,y,x,n] * a[s, y + ky - kh/2, x + kx - kw/2, c]      db[n] = sum_{s,y,x} dy[s,y,x,n]
 * with taps outside the H x W grid of the SAME sample contributing zero.  dy: 16-bit [S*H*W, N], pixel stride ld_dy >= N; a: 16-bit
 * [S, H, W, C], already normalised and activated, pixel stride ld_a >= C; strides in elements, multiples of 8; bases 16-byte aligned.
 * out_dtype: BG_F32 or `dtype`.  N % 128 == 0 and C % 128 == 0 (BG_E_SHAPE): a 128-column tile of dw then lies inside one tap, and
 * the loader's row for output pixel m is the pixel shifted by that tap, zero-filled in registers where it leaves the sample's grid
 * -- never read from memory, never taken from the neighbouring sample; no im2col matrix is written.  Otherwise bg_linear_wgrad's
 * kernel and rules with M = S*H*W and K = kh*kw*C: 128 x 128 tiles x slices of whole 32-pixel steps, split = 0 (auto: never an empty slice) or 1 .. 64
 * (a forced split beyond the row steps leaves trailing slices empty: zero partials), split > 1 through fp32 partials [split][N][K] then [split][N] in the workspace and bg_linear_wgrad's reduce
 * kernel; S == 0 writes zeros.  With fp32 output row n of dw depends on column n of dy alone; a non-finite dy[m, n] makes dw[n, :]
 * and db[n] non-finite (a GradScaler's found_inf trips) and leaves the other rows finite. */
int bg_conv_wgrad(const void* dy, int ld_dy, const void* a, int ld_a, void* dw, void* db, int S, int H, int W, int N, int C, int kh,
                  int kw, int dtype, int out_dtype, int split, void* workspace, size_t workspace_bytes, bg_stream_t stream);
/* 0 for split == 1 (or an auto split that resolves to 1), else 4 * split * N * (kh*kw*C + 1) rounded up to 256 bytes; 0 for rejected
 * arguments. */
size_t bg_conv_wgrad_workspace_bytes(int S, int H, int W, int N, int C, int kh, int kw, int split);
/* host-side plan, no device call: the split that 0 resolves to (1 for rejected arguments) */
int bg_conv_wgrad_split(int S, int H, int W, int N, int C, int kh, int kw);

/* src: an nn.Conv2d / nn.Conv1d weight [N, C, kh, kw] (fp32, or 16-bit of `dtype`) -> either or both of
 *     fwd   [N, kh*kw*C]   fwd[n, tap, c] = src[n, c, tap]                       the forward's (and bg_conv_wgrad's) layout
 *     dgrad [C, kh*kw*N]   dgrad[c, kh*kw - 1 - tap, n] = src[n, c, tap]         taps reversed, channels swapped
 * both 16-bit of `dtype`, round to nearest even: autocast's per-step weight cast.  A 'same' forward convolution of dy [.., N] with
 * dgrad is the data gradient of the convolution with src.  N % 32 == 0, C % 32 == 0, window odd and <= 5 x 5; dense, 16-byte
 * aligned.  One launch: 32 x 32 x kh*kw blocks through LDS. */
int bg_conv_weight_pack(const void* src, int src_dtype, int N, int C, int kh, int kw, void* fwd, void* dgrad, int dtype,
                        bg_stream_t stream);

/* Workspace of bg_gn_act_bwd: the fp64 partial sums [S][ceil(P / 64)][3][C], the fp64 sums [S][3][C] and the fp32 means [S][G][4], each
 * rounded up to 256 bytes; 0 for rejected shapes. */
size_t bg_gn_act_bwd_workspace_bytes(int S, int P, int C, int G);
/* The backward of a = act(GroupNorm(x)) as bg_im2col applies it (act: bg_vae_act -- none, SiLU, GELU-erf).  da, x, dx fp32 [S, P, C]
 * dense; stats [S, G, 2] as bg_groupnorm_stats wrote them; gamma, beta fp32 [C]; dskip fp32 [S, P, C] or NULL: the gradient that
 * arrives over the residual connection, added into dx in the same pass.  With
 *     xh = (x - mean) * rstd,   v = xh * gamma + beta,   dv = da * act'(v)
 * pass 1 writes sum_p dv, sum_p dv * xh and sum_p (x - mean) per (sample, channel) over chunks of 64 positions (within a chunk a chain takes every R-th
 * position, R = max(1, 256 / (C / 4))); the chains of a chunk, then the chunks, are added in index order.  All of it is fp64 from the
 * first term -- dv and xh are fp32 values, their product is exact in fp64 -- so no fp32 chain exists at all (fp32 chains of 32
 * positions missed the tests' yardstick at [2, 64, 512]).  From those: dbeta[c] = sum_s sum_p dv and dgamma[c] = sum_s sum_p dv * xh
 * (the samples in four contiguous quarters, in fp64, rounded once; both NULL = not computed, one NULL is BG_E_ARG) and per (sample,
 * group) m1 = mean(dv * gamma), m2 = mean(dv * gamma * xh) over P * C / G elements, rounded to fp32.  The third sum gives
 * delta = mean_group(x - mean), what the fp32 statistics' mean is off by (a few ulp of |mean|; with |mean| = 50 std the largest error of
 * this backward): the second sum is corrected by - delta * rstd * sum_p dv, and pass 2 forms xh = ((x - mean) - delta) * rstd.  Pass 2
 * writes every element of
 *     dx = rstd * fmaf(-xh, m2, fmaf(dv, gamma, -m1)) [+ dskip]       (= rstd * (dv * gamma - m1 - xh * m2), two roundings fewer)
 * -- with dskip, the bits of the call without it plus one fp32 add.  C % 4 == 0, G divides C, P >= 1, 1 <= S <= 65535 (BG_E_SHAPE);
 * 16-byte accesses, all bases 16-byte aligned (stats: 8).  Four launches (three without dgamma / dbeta), no host synchronisation. */
int bg_gn_act_bwd(const float* da, const float* x, const float* stats, const float* gamma, const float* beta, const float* dskip,
                  float* dx, float* dgamma, float* dbeta, int S, int P, int C, int G, int act, void* workspace, size_t workspace_bytes,
                  bg_stream_t stream);

/* ---- resampling convolutions in TRAINING (csrc/conv_train.hip): the backward of the VAEs' two 3 x 3 resampling convolutions,
 *   DOWN  diffusers Downsample2D   y = conv2d(F.pad(x, (0, 1, 0, 1)), w, stride = 2)            H, W even, Ho = H / 2, Wo = W / 2
 *         y[s,j,i,n] = b[n] + sum_{ky,kx,c} x[s, 2j + ky, 2i + kx, c] w[n,c,ky,kx]       a tap counts where 2j + ky < H and 2i + kx < W
 *   UP    diffusers Upsample2D     y = conv2d(F.interpolate(x, scale_factor = 2, mode = "nearest"), w, padding = 1)   Ho = 2H, Wo = 2W
 *         y[s,y,x,n] = b[n] + sum x[s, uy >> 1, ux >> 1, c] w[n,c,ky,kx],  uy = y + ky - 1, ux = x + kx - 1;  a tap counts where
 *         0 <= uy < 2H and 0 <= ux < 2W -- tested BEFORE the shift
 * whose forwards run on bg_im2col (stride / up / the before-padding) + bg_gemm_bias_act_fwd and bg_conv_gemm_fwd (up).  Activations are
 * channels-last, grids powers of two, 16-bit operands BG_BF16 | BG_F16, N and C multiples of 128.  No atomics, one writer per output
 * element, fixed summation order; arguments are checked before any launch.  UP's data gradient is the stride-1 'same' data gradient on
 * the 2H x 2W grid (above) followed by bg_pool2x2_sum. */
typedef enum { BG_CONV_SAME = 0, BG_CONV_DOWN2 = 1, BG_CONV_UP2 = 2 } bg_conv_geom;

/* bg_conv_wgrad in one of three geometries: H x W is the grid of `a` [S, H, W, C], dy has M = S*Ho*Wo rows (Ho x Wo: H x W | H/2 x W/2 |
 * 2H x 2W), dw is the forward pack's tap-major [N, 9C]:
 *     DOWN2   dw[n,(ky,kx),c] = sum_{s,j,i} dy[s,j,i,n] a[s, 2j + ky, 2i + kx, c]        where 2j + ky < H and 2i + kx < W
 *     UP2     dw[n,(ky,kx),c] = sum_{s,y,x} dy[s,y,x,n] a[s, uy >> 1, ux >> 1, c]        where 0 <= uy < 2H and 0 <= ux < 2W
 * and db[n] = sum dy[., n].  The same kernel with one more loader: the row staged for output pixel m is one pixel of `a` computed as
 * above, zero-filled in registers where the tap leaves the sample's grid -- never read, never taken from the neighbouring row or
 * sample.  geom = BG_CONV_SAME forwards to bg_conv_wgrad (the same bits).  Otherwise bg_conv_wgrad's rules, and: window 3 x 3 only,
 * BG_CONV_DOWN2 needs H, W >= 2 (BG_E_SHAPE); geom outside the enum is BG_E_ARG.  The split plan is lb_auto_split(M, N, 9C) with M
 * from dy's grid; workspace as bg_conv_wgrad's formula with that split. */
int bg_conv_wgrad_geom(const void* dy, int ld_dy, const void* a, int ld_a, void* dw, void* db, int S, int H, int W, int N, int C, int kh,
                       int kw, int geom, int dtype, int out_dtype, int split, void* workspace, size_t workspace_bytes, bg_stream_t stream);
size_t bg_conv_wgrad_geom_workspace_bytes(int S, int H, int W, int N, int C, int kh, int kw, int geom, int split);
int bg_conv_wgrad_geom_split(int S, int H, int W, int N, int C, int kh, int kw, int geom);

/* src: a 3 x 3 nn.Conv2d weight [N, C, 3, 3] (fp32, or 16-bit of `dtype`) -> either or both of
 *     fwd    [N, 9C]      bg_conv_weight_pack's forward pack
 *     down   9*C*N elements: the CLASS-ORDERED pack of bg_conv_down_dgrad, four dense blocks one after the other,
 *            block k = [C, T_k * N], block[c, t, n] = src[n, c, tap_k[t]], with the taps (ky, kx) of
 *            k = 0: (1,1) | k = 1: (1,0) (1,2) | k = 2: (0,1) (2,1) | k = 3: (0,0) (0,2) (2,0) (2,2)     (blocks start at C*N * {0, 1, 3, 5})
 * 16-bit of `dtype`, round to nearest even.  N % 32 == 0, C % 32 == 0; dense, 16-byte aligned.  One launch. */
int bg_conv_weight_pack_down(const void* src, int src_dtype, int N, int C, void* fwd, void* down, int dtype, bg_stream_t stream);

/* DOWN's data gradient: dx fp32 [S, H, W, C] from dy 16-bit [S, H/2, W/2, N] (pixel stride ld_dy >= N, a multiple of 8) and the
 * class-ordered pack:
 *     dx[s,iy,ix,c] = sum dy[s, (iy - ky) / 2, (ix - kx) / 2, n] w[n,c,ky,kx]   over ky in {1} for odd iy, {0, 2} for even iy, likewise kx,
 *                                                                               wherever iy - ky >= 0 and ix - kx >= 0
 * The four parity classes of (iy, ix) take 1, 2, 2 and 4 taps: 9 tap-products per four input pixels, the forward's work (no
 * zero-stuffed dy).  One gather launch writes the three multi-tap class operands [M, T_k * N] (M = S*H/2*W/2; a neighbour before the
 * sample's first row / column is zeros by an index test; class 0's operand is dy itself), four bg_gemm_bias_act_fwd launches fill a
 * class-major fp32 buffer [4][M][C], one 16-byte pass interleaves it into dx: every element of dx is written exactly once.  H, W
 * powers of two >= 2, S >= 1, N and C multiples of 128 (BG_E_SHAPE).  Workspace: the three operands and the buffer, each rounded up to
 * 256 bytes (2 * al(4MN) + al(8MN) + al(16MC) bytes); 0 for rejected shapes. */
size_t bg_conv_down_dgrad_workspace_bytes(int S, int H, int W, int N, int C);
int bg_conv_down_dgrad(const void* dy, int ld_dy, const void* pack, float* dx, int S, int H, int W, int N, int C, int dtype, void* workspace,
                       size_t workspace_bytes, bg_stream_t stream);

/* y[s,Y,X,c] = (u[s,2Y,2X,c] + u[s,2Y,2X+1,c]) + (u[s,2Y+1,2X,c] + u[s,2Y+1,2X+1,c]) (+ add[s,Y,X,c]), fp32, in that association:
 * the backward of nearest x2 up-sampling.  u [S, 2H, 2W, C], y and add (may be NULL: e.g. a skip gradient) [S, H, W, C], dense,
 * 16-byte aligned, C % 4 == 0.  One launch, 16-byte accesses. */
int bg_pool2x2_sum(const float* u, const float* add, float* y, int S, int H, int W, int C, bg_stream_t stream);

/* QKV projection with the LayerNorm fold + self-attention in ONE launch (csrc/qkv_attn.hip): sequences of an even length
 * N <= 64, all B of them equally long; key_pad (may be NULL) as bg_attn_fwd's.  x_hi [B*N, 768] raw 16-bit rows, w_qkv [2304, 768] /
 * bias / colsum as bg_gemm_ex_fwd's fold operands, stats_in [12][B*N][2] the row statistics partials of x; out [B*N, 768] = what
 * bg_gemm_ex_fwd followed by bg_attn_fwd produce, bit for bit.  qkv_dbg (tests; may be NULL): [B*N, 2304] receives the q|k|v of
 * that GEMM. */
int bg_qkv_attn_fwd(const void* x_hi, const void* w_qkv, const float* bias, const float* colsum, const float* stats_in,
                    const uint8_t* key_pad, void* out, void* qkv_dbg, int B, int N, int dtype, float ln_eps, bg_stream_t stream);
/* FFN1 (LayerNorm fold, ReLU) + FFN2 (split residual in place + row statistics) of one encoder layer in ONE launch
 * (csrc/ffn_fused.hip; network.py:1076-1078, dim_feedforward = 1024): the residual planes x_hi / x_lo [M, 768] (16-bit, dtype) are
 * updated in place, stats [12][m_stride][2] holds the row-statistics partials of x on entry and those of the new x on return;
 * w1_frag / w2_frag: bg_layer_weights.w_1f / w_2f; b1 / colsum1: the fold's bias and column sums [1024]; b2 [768].  m_dev (may be
 * NULL): device-side row count <= M.  Bit for bit what bg_gemm_ex_fwd (fold, ReLU) followed by bg_gemm_ex_fwd (split residual +
 * statistics) produce. */
int bg_ffn_fused_fwd(void* x_hi, void* x_lo, float* stats, const void* w1_frag, const float* b1, const float* colsum1,
                     const void* w2_frag, const float* b2, int M, int m_stride, const int* m_dev, int dtype, float ln_eps,
                     bg_stream_t stream);
/* The same launch on a SLOT-PACKED ragged batch (bg_compact_rows_paired): *m_dev rows (device-side, a multiple of 64) in 64-row
 * slots of one or two whole samples, slot_desc[2 k] / [2 k + 1] their lengths, at most slot_bound slots; m_stats = row stride of
 * stats_in.  out rows = what bg_gemm_ex_fwd + bg_attn_varlen_fwd produce for the same samples on the dense packing, bit for bit.
 * Invariants the kernel TRUSTS (bg_compact_rows_paired guarantees them; nothing on the device re-checks): *m_dev <= 64 * slot_bound
 * and a multiple of 64; slot_desc[2 k] >= 1, slot_desc[2 k] + slot_desc[2 k + 1] <= 64 for every slot below *m_dev / 64;
 * slot_bound <= 43 690 (32-bit row offsets; rejected above). */
int bg_qkv_attn_paired_fwd(const void* x_hi, const void* w_qkv, const float* bias, const float* colsum, const float* stats_in,
                           void* out, void* qkv_dbg, const int* m_dev, const int* slot_desc, int slot_bound, int m_stats,
                           int dtype, float ln_eps, bg_stream_t stream);
/* The tail of the denoisers' output MLP in one launch (csrc/out_tail.hip): out[m, :n_out] = W3 . SiLU(LayerNorm(t0[m, :])) + b3 with
 * t0 [rows, 768] 16-bit rows of `dtype`, w3 [n_out_pad, 768] of the same dtype (the first 16 * ceil(n_out / 16) rows are read),
 * b3 fp32 [n_out_pad], 1 <= n_out <= 48, out fp32 [rows, n_out]. */
int bg_ln_silu_out_fwd(const void* t0, const float* ln_g, const float* ln_b, const void* w3, const float* b3, float* out,
                       int n_out, int n_out_pad, int rows, int dtype, float eps, bg_stream_t stream);
/* Slot-packed compaction for samples of at most 64 tokens (mask [B, n_mask], 1 = padded): every 64-row slot holds one or two whole
 * samples (shortest joins longest while the sum fits), the rows behind them are clones of the slot's first row.  offsets [B + 1]:
 * first row of every sample, offsets[B] = 64 * slots (stays on the device); src_row [64 B]; slot_desc [2 B]; slot_a [B]: the first
 * sample of every slot; counts [B]: scratch. */
int bg_compact_rows_paired(const uint8_t* mask, int B, int n_mask, int* offsets, int* src_row, int* slot_desc, int* slot_a,
                           int* counts, bg_stream_t stream);
/* Valid-token compaction behind the variable-length execution (csrc/compact.hip): mask uint8 [B, n_mask] (1 = padded),
 * each entry covering `rep` consecutive tokens (EdgePosNet: one entry per face, rep = E).  Writes offsets int32 [B+1]
 * (offsets[B] = number of valid tokens; it stays on the device) and src_row int32 [B*n_mask*rep]: the padded-layout index of
 * every compact row, in order (entries past offsets[B] are not written). */
int bg_compact_rows(const uint8_t* mask, int B, int n_mask, int rep, int* offsets, int* src_row, bg_stream_t stream);

/* ---- whole denoiser -------------------------------------------------------------------- */

typedef struct {            /* Linear(k_in,768) -> LayerNorm -> SiLU -> Linear(768,n_out)   (sub-keys .0 .1 .3) */
    const void* w0;         /* [768,k_in]; fp32 for the input/time embeds (tiny K or M: exact fp32 MFMA),
                               compute dtype for fc_out (K = 768, M = all tokens) */
    const float* b0;
    const float* ln_g;
    const float* ln_b;
    const void* w3;         /* compute dtype [n_out_pad,768] */
    const float* b3;        /* fp32 [n_out_pad] */
    int k_in, n_out, n_out_pad, w0_dtype;
    const float* w0_mfma;   /* optional, k_in in {6,12,48} with fp32 w0: W0 in MFMA operand order,
                               [24][k_in/2][64] with element (ct, kk, lane) = w0[ct*32 + (lane & 31)][2*kk + (lane >> 5)]:
                               selects the fused Linear + LayerNorm + SiLU kernel (bg_embed_ln_silu_fwd) */
    const float* w0_colsum; /* fc_out only (16-bit modes with the LayerNorm fold; NULL elsewhere): the encoder's final LayerNorm
                               (net.norm) is folded into fc_out.0 -- w0 = T(net.norm.weight * W0), b0 = b0 + W0 net.norm.bias,
                               w0_colsum[n] = sum_k float(w0[n,k]) -- and the rest of the MLP (LayerNorm + SiLU + Linear(768, n_out))
                               runs as one launch (bg_ln_silu_out_fwd) */
} bg_mlp_weights;

typedef struct {            /* one nn.TransformerEncoderLayer (norm_first) */
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    const void* w_qkv;      /* [2304,768], q rows pre-scaled by 1/8 */
    const float* b_qkv;     /* q part pre-scaled */
    const void* w_o;        /* [768,768]  */
    const float* b_o;
    const void* w_1;        /* [1024,768] */
    const float* b_1;
    const void* w_2;        /* [768,1024] */
    const float* b_2;
    /* LayerNorm fold (16-bit compute dtypes; both NULL = unfolded: the two LayerNorms run as kernels).  When set,
     * w_qkv = T(norm1.weight * W_in) and b_qkv = b_in + W_in norm1.bias (q parts pre-scaled), likewise w_1 / b_1 with
     * norm2, and *_colsum[n] = sum_k float(w[n,k]) of the ROUNDED folded weights; the GEMM then takes the raw 16-bit
     * residual rows and applies mean / rstd per row in its epilogue. */
    const float* qkv_colsum; /* fp32 [2304] */
    const float* w1_colsum;  /* fp32 [1024] */
    /* optional (ABI 6; both NULL = FFN1 and FFN2 stay two launches): the SAME folded w_1 / w_2 once more, in MFMA fragment order for
     * bg_ffn_fused_fwd (one launch per layer for FFN1 + ReLU + FFN2 + residual, the hidden tensor never leaves the CU):
     *   w_1f[w][s][j][lane][e] = w_1[(4 w + j) * 32 + (lane & 31)][16 s + 8 (lane >> 5) + e]   w < 8, s < 48, j < 4, lane < 64, e < 8
     *   w_2f[w][s][j][lane][e] = w_2[(3 w + j) * 32 + (lane & 31)][16 s + 8 (lane >> 5) + e]   w < 8, s < 64, j < 3 */
    const void* w_1f;
    const void* w_2f;
} bg_layer_weights;

typedef struct {
    int net;                /* enum bg_net */
    int dtype;              /* GEMM/attention operand dtype: BG_BF16 or BG_F32 */
    int n_layer;            /* 12 */
    int _pad;
    bg_layer_weights layers[BG_MAX_LAYERS];
    const float *lnf_g, *lnf_b;            /* net.norm */
    bg_mlp_weights time_embed;
    bg_mlp_weights fc_out;
    /* SurfPos: {p_embed}; SurfZ: {z_embed,p_embed}; EdgePos: {surfp,surfz,edgep};
     * EdgeZ: {surfp,surfz,edgep,edgez,vertp} */
    bg_mlp_weights embed[BG_MAX_EMBEDS];
    const float* class_embed;              /* fp32 [11,768] or NULL (use_cf=False) */
    /* optional: the time-embedding MLP (sincos -> time_embed) evaluated once for t = 0 .. time_table_rows - 1, fp32
     * [time_table_rows, 768] -- a function of the weights only; with it an evaluation looks its timestep(s) up instead of running
     * the five small launches of that MLP (a timestep outside the table yields NaN).  NULL: computed per call. */
    const float* time_table;
    int time_table_rows;
    int _pad3;
} bg_denoiser_weights;

typedef struct {
    int B, S, E;            /* E = 1 for the surface nets; tokens per sample N = S*E */
    int n_timesteps;        /* 1 (sampling) or B (training-style per-sample t) */
    const float* x;         /* noisy input: SurfPos [B,S,6] | SurfZ [B,S,48] | EdgePos [B,S,E,6] | EdgeZ [B,S,E,18] */
    const float* surf_pos;  /* [B,S,6]   (SurfZ, EdgePos, EdgeZ) */
    const float* surf_z;    /* [B,S,48]  (EdgePos, EdgeZ) */
    const float* edge_pos;  /* [B,S,E,6] (EdgeZ) */
    const uint8_t* mask;    /* 1 = padded. SurfZ/EdgePos: [B,S]; EdgeZ: [B,S,E]; SurfPos: NULL */
    const int64_t* timesteps;
    const int64_t* class_label;  /* [B] or NULL */
    float* cond_cache;      /* optional [B*S,768] fp32: step-invariant conditioning embeds */
    int cond_cache_valid;   /* 1: reuse cond_cache, 0: (re)compute and store if cond_cache != NULL */
    /* Variable-length execution (needs mask): the valid tokens of every sample are packed into consecutive rows, all
     * GEMM / LayerNorm work runs on sum(valid) rows, attention runs per sample over its own rows, eps_out is the padded
     * layout with 0 at padded positions.  Valid positions are unchanged up to rounding (a padded token is never a key
     * of a valid query: network.py:1196, 1283, 1390); the reference computes -- and discards, sample.py:284, 307-314 --
     * values at padded positions.  The row count stays on the device: no host synchronisation. */
    int varlen;
    /* Host-side ESTIMATE of the number of valid tokens / of the sum over samples of valid^2 (variable-length execution; 0 =
     * unknown).  The row count that the kernels use is always the one counted on the device; the estimate only (a) lets the GEMM
     * launcher choose between "256 x 256 + 128 x 128 kernels, split rule evaluated on the device" and "128 x 128 kernel alone"
     * -- either choice is correct for ANY actual count, and the results are bit-identical -- and (b) is what the opt-in profiler
     * (bg_profile_*) books as executed FLOPs / bytes.  With 0 the launcher plans for the bound B * S * E and the profiler books
     * the padded sizes. */
    double rows_hint, pairs_hint;
    /* Software pipelining over independent sub-batches: n_split in 2..4 cuts the batch into that many contiguous
     * groups of samples and runs their forwards concurrently -- the first on `stream`, the others on helper streams
     * forked from it and joined back into it by events before the call returns (HIP-graph capturable).  Every op of the
     * path is per-sample and every kernel bit-stable across batch sizes, so the result is identical; what it buys is
     * occupancy: the tile-round tails and the memory-bound epilogues of one group hide under the K loops of another.
     * 0 / 1 = off; negative values are rejected.  The helper streams and events are created lazily, once per DEVICE (a process
     * that drives several devices gets one set each), and used under a mutex (enqueue only). */
    int n_split;
    int _pad2;
    /* Optional (variable-length execution; 0 = not known): the row count the kernels of sample group k WILL see -- the valid tokens of
     * the group, or 64 x its slots where the batch runs slot-packed -- when the caller knows it exactly ([0] alone without n_split).
     * Like rows_hint it only chooses between launch plans that are all correct for any actual count (the device still counts); what an
     * exact count buys is launches that are not made: a GEMM whose rows all belong to the 256 x 256 kernel is ONE launch instead of that
     * kernel + a 128 x 128 tail kernel that finds nothing to do (4-5 us each, twice per encoder layer on the face LDM's ragged loop). */
    double rows_plan[4];
} bg_denoiser_inputs;

/* 1 when a variable-length call of bg_denoiser_fwd with these shapes runs SLOT-PACKED (64-row slots of one or two samples, the fused QKV +
 * attention launch): the library's own predicate (net, shapes, 16-bit dtype, LayerNorm-fold weights given = `fold`, BG_TUNE_QKV_ATTN),
 * exported so that a host that fills bg_denoiser_inputs.rows_plan counts the rows of the layout the library will actually use.
 * rows_plan only ever chooses between launch plans that are all correct for any row count: it must never be used to skip work. */
int bg_slot_packing_applies(int net, int B, int S, int E, int dtype, int fold);

/* bytes of scratch bg_denoiser_fwd needs for these shapes (sized so that any n_split <= 4 fits) */
size_t bg_workspace_bytes(int net, int B, int S, int E, int dtype);

/* {SurfPosNet,SurfZNet,EdgePosNet,EdgeZNet}.forward -- network.py:1107-1126,1176-1200,1257-1286,
 * 1357-1393.  eps_out fp32, shaped like in->x. */
int bg_denoiser_fwd(const bg_denoiser_weights* w, const bg_denoiser_inputs* in, float* eps_out,
                    void* workspace, size_t workspace_bytes, bg_stream_t stream);

/* Pieces of the whole-net call on their own (same kernels, caller-owned 256-byte-aligned scratch):
 *   bg_embed_mlp_fwd      Linear(k,768) -> LayerNorm -> SiLU -> Linear(768,n) (+ add[m / add_div]) of one bg_mlp_weights
 *                         (network.py:1080-1099); x fp32 rows (input embeds) or `dtype` rows (fc_out); out fp32.
 *   bg_encoder_layer_fwd  one nn.TransformerEncoderLayer(768, 12, norm_first=True, dim_feedforward=1024) (network.py:
 *                         1076-1078) on an fp32 residual stream x [B*N,768], in place; key_pad uint8 [B,N] or NULL.  Takes
 *                         UNFOLDED layer weights (qkv_colsum == w1_colsum == NULL): the LayerNorm-folded, split-residual
 *                         formulation of the 16-bit modes keeps state between layers and lives inside bg_denoiser_fwd. */
size_t bg_embed_mlp_scratch_bytes(int rows, int dtype);
int bg_embed_mlp_fwd(const bg_mlp_weights* m, int dtype, const void* x, int lda, int rows, float* out, int ldc,
                     const float* add, int ld_add, int add_div, void* scratch, size_t scratch_bytes, bg_stream_t stream);
size_t bg_encoder_layer_scratch_bytes(int B, int N, int dtype);
int bg_encoder_layer_fwd(const bg_layer_weights* L, int dtype, float* x, const uint8_t* key_pad, int B, int N,
                         void* scratch, size_t scratch_bytes, bg_stream_t stream);

/* ---- scheduler steps (diffusers==0.27 arithmetic, called at sample.py:137,153,202,222,236,282) */

/* DDPMScheduler.step fused with the classifier-free-guidance combine (sample.py:132-134):
 *   eps = eps_c*(1+w) - eps_u*w   (eps_u NULL -> eps = eps_c)
 *   x0  = clamp((x - sqrt_beta_prod*eps) / sqrt_alpha_prod, +-clip)   (clip <= 0: no clamp; as torch.clamp: NaN stays NaN)
 *   out = x0_coeff*x0 + xt_coeff*x + sigma*noise                      (noise NULL or sigma==0: skipped)
 * scalars are computed on the host in fp32 (brepgen_amd.schedulers).  n = element count. */
int bg_cfg_ddpm_step(const float* eps_c, const float* eps_u, float guidance_w, const float* x,
                     const float* noise, float* out, size_t n, float sqrt_alpha_prod,
                     float sqrt_beta_prod, float x0_coeff, float xt_coeff, float sigma, float clip,
                     bg_stream_t stream);

/* PNDMScheduler.step (PRK + PLMS) as one fused pass.
 *   e      = eps_c*(1+w) - eps_u*w
 *   if store_e:  e_store = e                       (PRK phase 0 / every PLMS step: the `ets` history)
 *   comb   = c_e*e + c_acc*acc + sum_i c_hist[i]*hist[i]
 *   if acc_mode==1: acc_out = acc_scale_old*acc + acc_scale_e*e    (PRK running cur_model_output)
 *   out    = sample_coeff*x - eps_coeff*comb
 */
int bg_pndm_step(const float* eps_c, const float* eps_u, float guidance_w, const float* x,
                 float* e_store, const float* acc, float* acc_out, float acc_scale_old,
                 float acc_scale_e, float c_e, float c_acc, const float* hist0, const float* hist1,
                 const float* hist2, float c_h0, float c_h1, float c_h2, float sample_coeff,
                 float eps_coeff, float* out, size_t n, bg_stream_t stream);

/* ---- VAE steps (AutoencoderKLFastDecode / AutoencoderKL1DFastDecode / ...FastEncode, network.py:690-1040; blocks from
 * diffusers==0.27).  Channels-last fp32 activations [S, H, W, C] (1-D: H = 1).  A convolution is either bg_im2col with a
 * 1x1 window (GroupNorm + activation + cast) followed by the implicit GEMM bg_conv_gemm_fwd, or bg_im2col over the whole
 * window followed by bg_gemm_bias_act_fwd, on weights reshaped to [C_out, kh*kw*C_in]; bg_vae_run (below) strings a whole
 * pass together. ------------------------------------------------------------------------------------------------- */

/* nn.GroupNorm statistics: stats[s, g] = (mean, 1/sqrt(var + eps)) over the P positions x C/G channels of group g. */
int bg_groupnorm_stats(const float* x, float* stats /*[S,G,2]*/, int S, int P, int C, int G, float eps,
                       bg_stream_t stream);

/* im2col of a kh x kw convolution with `stride`, over the logical input grid (Hin << up, Win << up), producing
 * an Ho x Wo output grid; `pad_y` / `pad_x` zeros precede the first row / column, whatever the window needs beyond
 * the last row / column is zero as well (covers pad=1 convs, and Downsample2D's F.pad(0,1,0,1) + stride 2).  With
 *   - optional nearest x2 up-sampling of the source (Upsample2D) folded in (up = 1),
 *   - optional GroupNorm (stats from bg_groupnorm_stats, gamma, beta) and activation (0 none, 1 SiLU, 2 GELU-erf)
 *     applied on the fly (ResnetBlock2D / ResConvBlock / conv_norm_out),
 *   - optional residual `add` [S*Ho*Wo, C] added after the activation (1x1 window only: the tail of ResConvBlock).
 * out: [S*Ho*Wo, kh*kw*C] fp32 / bf16 / fp16, tap-major / channel-minor. */
int bg_im2col(const float* x, void* out, int out_dtype, int S, int Hin, int Win, int C, int kh, int kw, int up,
              int stride, int pad_y, int pad_x, int Ho, int Wo, const float* stats, const float* gamma,
              const float* beta, int G, int act, const float* add, bg_stream_t stream);

/* diffusers Upsample1d("cubic") (network.py:43): x [S,L,C] -> y [S,2L,C], reflect pad + 8-tap transposed conv. */
int bg_upsample1d_cubic(const float* x, float* y, int S, int L, int C, bg_stream_t stream);

/* diffusers Downsample1d("cubic") of the edge encoder (network.py:86-185 via get_down_block): [S,L,C] -> [S,L/2,C]. */
int bg_downsample1d_cubic(const float* x, float* y, int S, int L, int C, bg_stream_t stream);

/* Self-attention of the VAE mid blocks (diffusers Attention with 1 head over 16 tokens; SelfAttention1d with
 * C/32 heads over 4 tokens): qkv fp32 [S*T, ld] with q|k|v at columns 0, C, 2C; out [S*T, C] fp32 or bf16. */
int bg_small_attn(const float* qkv, int ld, void* out, int out_dtype, int S, int T, int C, int nh, float scale,
                  bg_stream_t stream);

/* ---- a whole VAE pass as ONE call (bg_vae2d_decode / bg_vae1d_decode; the encoders too).
 * Replaces AutoencoderKLFastDecode / AutoencoderKL1DFastDecode / ...FastEncode.forward (network.py:690-1040): the four
 * networks are the same few steps in different orders, so there is one interpreter and the caller hands it the
 * network as a flat program (brepgen_amd/vae.py builds it once per module and dtype from the state dict).  Every
 * launch of the pass is enqueued on `stream` by this call; nothing is allocated and nothing synchronises.
 *
 * Activations live in SLOTS: fp32 channels-last [S, H, W, C] (1-D: H = 1).  Slot 0 is the caller's input, slot
 * BG_VAE_OUT the caller's output, slots 1 .. n_slots-1 are carved from the workspace (all the same size: the largest
 * activation of the program).  A step reads `src` (+ optional residual `res`) and writes `dst` (dst != src, res).
 *   BG_VOP_CONV          [GroupNorm (+act) ->] conv kh x kw [on the nearest-x2 up-sampled grid: up = 1] [stride 2] + bias
 *                        [+ res].  pad_mode 0: "same" zero padding (kh/2, kw/2); 1: Downsample2D's F.pad(0,1,0,1), no other.
 *                        w: [n_pad, kh*kw*C_in] tap-major / channel-minor, dtype w_dtype; columns < n_out are written.
 *                        Runs as the implicit GEMM bg_conv_gemm_fwd when that kernel's shape rules hold, else
 *                        bg_im2col + bg_gemm_bias_act_fwd -- the same choice for the same shapes, so results do not
 *                        depend on how the batch is chunked beyond which of the two a chunk size selects.
 *   BG_VOP_NORM_ACT_ADD  dst = act(GroupNorm(src)) + res                     (the tail of diffusers' ResConvBlock)
 *   BG_VOP_ATTN          dst = src + proj(softmax(q k^T * scale) v), q|k|v = GroupNorm(src) w^T + bias ([3C, C] fused),
 *                        per sample over its H*W tokens with `heads` heads; w2 / bias2 = the output projection
 *   BG_VOP_UP1D / DOWN1D bg_upsample1d_cubic / bg_downsample1d_cubic
 * The batch is processed in chunks of `chunk` samples; bg_vae_workspace_bytes(n, chunk) is the workspace that takes. */
enum bg_vae_opcode { BG_VOP_CONV = 0, BG_VOP_NORM_ACT_ADD = 1, BG_VOP_ATTN = 2, BG_VOP_UP1D = 3, BG_VOP_DOWN1D = 4 };
enum bg_vae_act { BG_VACT_NONE = 0, BG_VACT_SILU = 1, BG_VACT_GELU = 2 };
#define BG_VAE_MAX_SLOTS 8
#define BG_VAE_OUT 255
typedef struct {
    int op;                    /* bg_vae_opcode */
    int src, dst, res;         /* slots; res = -1: none */
    int kh, kw, up, stride, pad_mode;
    int n_out, n_pad, w_dtype; /* CONV: output channels, rows of w, BG_F32 | BG_BF16 | BG_F16.  ATTN: n_pad / w_dtype of the q|k|v weights */
    const void* w;
    const float* bias;
    const float* gn_gamma;     /* NULL: no GroupNorm in front */
    const float* gn_beta;
    int gn_groups;
    float gn_eps;
    int act;                   /* bg_vae_act, applied after the GroupNorm */
    int heads;                 /* ATTN */
    float scale;
    int n_pad2, w2_dtype;
    const void* w2;
    const float* bias2;
} bg_vae_op;
size_t bg_vae_workspace_bytes(const bg_vae_op* ops, int n_ops, int n_slots, int in_h, int in_w, int in_c, int n, int chunk);
/* x: [n, in_h, in_w, in_c] fp32; out: [n, Ho, Wo, C_out] fp32 (the shape of the step that writes BG_VAE_OUT);
 * zero_page: >= 2 * max C bytes of zeros (see bg_conv_desc); workspace 256-byte aligned. */
int bg_vae_run(const bg_vae_op* ops, int n_ops, int n_slots, int in_h, int in_w, int in_c, const float* x, int n, int chunk,
               float* out, const void* zero_page, void* workspace, size_t workspace_bytes, bg_stream_t stream);

/* ---- bbox de-duplication between the cascade stages, on the device (the reference does it on the host in numpy:
 * sample.py:159-183 faces, 242-261 edges).  Same greedy order-dependent algorithm in float32, incl. the
 * corner-swapped match and (faces) np.round(x, 4); decisions are bit-identical to the numpy code. */
int bg_dedup_surfaces(const float* surf_pos /*[B,S,6]*/, float threshold, float* pos_out /*[B,S,6] kept, 0-padded*/,
                      uint8_t* mask_out /*[B,S] 1 = padding*/, int B, int S, bg_stream_t stream);
int bg_dedup_edges(const float* edge_pos /*[B,S,E,6]*/, const uint8_t* surf_mask /*[B,S]*/, float threshold,
                   uint8_t* edge_mask /*[B,S,E] 1 = padded face or duplicate edge*/, int B, int S, int E,
                   bg_stream_t stream);

/* ---- measurement aid (bench.py's roofline leg): hipEvent pairs around every kernel launch ------------
 * bg_profile_begin allocates up to max_launches event pairs and switches recording on (this is the one
 * place the library owns state; it is off by default and costs nothing when off).  bg_profile_end
 * synchronises, aggregates per kernel and frees the events.  flops / bytes are the ALGORITHMIC counts the
 * launcher derives from the shapes (DESIGN.md "roofline accounting"). */
typedef struct {
    const char* kernel;     /* static string */
    int launches;
    double total_ms;        /* sum of launch durations */
    double flops;           /* sum of algorithmic FLOPs */
    double bytes;           /* sum of algorithmic HBM bytes */
} bg_profile_row;
int bg_profile_begin(int max_launches);
int bg_profile_end(bg_profile_row* rows, int max_rows);   /* returns the number of rows written (<0: error) */

/* ---- the path's one collective (batch sharding + ONE all-gather of the finished latents) ----
 * recv[r * bytes_per_rank ...] = rank r's `send` (bytes_per_rank bytes each; device pointers; every rank passes the same size -- the
 * Python host pads the last shard, brepgen_amd/sampling.py: gather_latents), enqueued on `stream`: a thin ncclAllGather (RCCL over
 * xGMI) on a communicator the CALLER created with ncclCommInitRank (`nccl_comm` = the ncclComm_t).  For hosts without
 * torch.distributed; the Python host uses all_gather_into_tensor on the "nccl" (= RCCL) backend, which is the same collective.
 * RCCL is dlopen'ed at the first call; returns 0, BG_E_ARG, or 1000 + ncclResult_t. */
int bg_allgather(const void* send, void* recv, size_t bytes_per_rank, void* nccl_comm, bg_stream_t stream);

/* Kernel-selection knobs.  Every choice computes bit-identical results: the keys exist so that the parity tests can run the same
 * work on each kernel that may serve it, and so that two kernels can be timed against each other in one process (value 0 always =
 * the library's own choice; process-global, not for production use).  The numbers are frozen: they appear in recorded logs and in
 * BG_TUNE strings.  bg_tune_set refuses every key that has no enumerator here with BG_E_ARG; values are not constrained. */
enum bg_tune_key {
    /* split-residual launches on the 256 x 256 kernel: start delay of the second phase group, x 1024 cycles (< 0: none) */
    BG_TUNE_GEMM_STAGGER = 8,
    /* 256 x 256 persistent kernel: 1 = alone wherever eligible, 2 = never */
    BG_TUNE_P256_MODE = 10,
    /* split-residual GEMMs of the encoder layers: 1 = the 128 x 128 persistent kernel instead of the pipelined one */
    BG_TUNE_SPLIT_PIPE = 12,
    /* QKV + attention of short, equally long sequences: 1 = as two launches (GEMM, attention) instead of the fused kernel, 2 = fused
     * wherever eligible (the library's own choice leaves a nearly empty second round of tiles to the two launches) */
    BG_TUNE_QKV_ATTN = 13,
    /* tile walk of that fused kernel: 1 = plain (every XCD runs all 12 heads), 2 = XCD-pinned head halves wherever the grid allows
     * (the library's own choice: from two rounds of tiles on) */
    BG_TUNE_QKV_WALK = 14,
    /* small launches: tile-count threshold of the 64 x 64-tile path (< 0: off) */
    BG_TUNE_SMALL_TILES = 15,
    /* FFN1 / FFN2 of layers that carry w_1f / w_2f: 1 = as two GEMM launches instead of the fused launch (bg_ffn_fused_fwd) */
    BG_TUNE_FFN_FUSED = 16,
    /* bg_vae_run, GroupNorm(1, C) over samples of 2048 / 4096 values (the 1-D VAE's blocks): 1 = statistics pass + gather as two
     * launches (bg_groupnorm_stats, bg_im2col) instead of the one-pass kernel */
    BG_TUNE_VAE_GN1_FUSED = 19,
    /* long-sequence attention: 1 = each XCD walks a contiguous eighth of the (sample, head) units (rounds 2-5) instead of the units
     * going round-robin over the XCDs (ragged batches: the eighths' shares of sum n_b^2 differ, the launch lasts as long as the
     * heaviest) */
    BG_TUNE_ATTN_WALK = 20
};
int bg_tune_set(int key, int value);

/* How a 16-bit GEMM launch of `rows` x `n_cols` (n_cols a multiple of 256) is partitioned between the 256 x 256
 * persistent kernel (rows [0, return value)) and the 128 x 128 one (the rest): the rule both kernels evaluate on the
 * device-side row count and the launcher evaluates on the host ("tile-round quantisation").
 * split_residual: the out-proj / FFN2 epilogue; concurrent: launches of sibling sample groups are in flight
 * (all-or-nothing).  No device work; usable without a GPU.  <0: error code. */
int bg_gemm_p256_rows(int rows, int n_cols, int split_residual, int concurrent);

/* DDPMScheduler.add_noise (training-time forward diffusion, trainer.py:348,399,515,...):
 *   out[b,:] = sqrt_alpha_prod[b] * x0[b,:] + sqrt_one_minus_alpha_prod[b] * noise[b,:]
 * the two per-sample scalar vectors are device fp32 [B] (gathered from alphas_cumprod by the host shim). */
int bg_add_noise(const float* x0, const float* noise, const float* sqrt_alpha_prod,
                 const float* sqrt_one_minus_alpha_prod, float* out, int B, size_t per_sample,
                 bg_stream_t stream);

/* Ancestral noise of the DDPM loops (the reference draws it on the device with the global RNG, sample.py:144-153 ->
 * diffusers randn_tensor(device=...)): out[b, e] ~ N(0,1) for samples b = 0 .. n_samples-1 of `per_sample` elements,
 * Philox4x32-10 with key = seed, counter = (e / 4, first_sample + b, draw_id, tag) and Box-Muller on the four words.
 * The value of an element depends only on (seed, draw_id, GLOBAL sample index, e): a rank that owns samples
 * [lo, hi) of a sharded batch passes first_sample = lo and reproduces exactly those rows of the single-GPU draw.
 * raw_bits != 0 writes the four 32-bit words themselves (bit pattern in the float slots) -- used by the parity test. */
int bg_philox_randn(float* out, long long n_samples, int per_sample, unsigned long long seed, unsigned draw_id,
                    long long first_sample, int raw_bits, bg_stream_t stream);

/* Device loop of joint_optimize (utils.py:746-772): per-face 3-D offsets fitted with `iters` AdamW steps (torch.optim.AdamW
 * arithmetic; the reference uses lr 1e-3, betas (0.95, 0.999), weight_decay 1e-6, eps 1e-8, 200 iterations) on
 *   L = mean_f sum_{e in edges_f} min_{s in surf_f} |e - (s + off_f)|^2        (chamferdist ChamferDistance(reverse=True)).
 * surf [F,P,3] (P <= 4096), edge_pts [edge_off[F],3] with face f owning rows edge_off[f] .. edge_off[f+1]-1 (int32, device).
 * offsets_out [F,3] and surf_out [F,P,3] (optional) are those of the LAST evaluated iteration (what the reference returns,
 * utils.py:770); loss_out [F] (optional) the per-face Chamfer sums of that iteration.  One launch, deterministic. */
int bg_chamfer_offset_fit(const float* surf, const float* edge_pts, const int* edge_off, int F, int P, int iters, double lr,
                          double beta1, double beta2, double weight_decay, double eps, float* offsets_out, float* surf_out,
                          float* loss_out, bg_stream_t stream);

/* Masked MSE of the trainers' loss / validation forward (trainer.py:354, 538, 597, 950-952; `loss_fn(pred[~mask],
 * noise[~mask])`): pred / target fp32 [rows, ld], row_mask uint8 [rows] (1 = padded, skipped) or NULL, columns
 * [col0, col0+ncols).  scratch: 1024 doubles.  out3 (device): {mean over valid elements, sum over valid rows of the
 * per-row mean (the reduction of test_val, trainer.py:597), number of valid rows}.  A row is summed in fp32 over pieces of 64 columns
 * and in fp64 across pieces and rows, so a whole sample can be one row (the VAE trainers, trainer.py:85, 122: rows = samples, no
 * mask).  Deterministic (no atomics). */
int bg_masked_mse(const float* pred, const float* target, const uint8_t* row_mask, long long rows, int ld, int col0,
                  int ncols, double* scratch, float* out3, bg_stream_t stream);

/* ---- evaluation metrics (pc_metric.py: COV / MMD / JSD over sets of point clouds) -------------------------------- */

/* Pairwise Chamfer matrix of `_pairwise_CD` (pc_metric.py:45-80, the `chamfer_distance` CUDA extension's dl.mean(1) + dr.mean(1);
 * the same quantity as the pure-torch distChamfer, pc_metric.py:32-42):
 *   out[i, j] = (1/Pa) sum_p min_q |a_ip - b_jq|^2 + (1/Pb) sum_q min_p |a_ip - b_jq|^2
 * a [S,Pa,3], b [R,Pb,3] fp32 contiguous, out [S,R] fp32; any S, R, Pa, Pb >= 1 with S * R < 2^31.  Direct-form fp32 distances
 * (|dx|^2 then two fused multiply-adds), no floating-point atomics, fixed summation order: out[i, j] depends bitwise on cloud a_i
 * and cloud b_j alone, not on S, R or the rest of the batch.  Coordinates must be finite.  One launch per 2^22 cloud pairs (one in all
 * for the reference's 3000 x 1000). */
int bg_chamfer_pairwise(const float* a, int S, int Pa, const float* b, int R, int Pb, float* out, bg_stream_t stream);

/* Occupancy-grid counts of `entropy_of_occupancy_grid` (pc_metric.py:110-149) on the res^3 product grid of
 * `unit_cube_grid_point_cloud`: pts [n_clouds,P,3] fp32, axis [res] fp32 ascending node coordinates (the host evaluates
 * i * spacing - 1 in double and rounds to fp32, as the reference's grid does), res <= 64.  point_counts / cloud_counts [res^3]
 * uint32, ZEROED BY THE CALLER, cell index (ix*res + iy)*res + iz:
 *   point_counts[c] += number of points whose nearest node is c           (the reference's grid_counters)
 *   cloud_counts[c] += number of clouds with at least one such point      (grid_bernoulli_rvars)
 * Per axis the nearest node is decided by comparing |x - axis[i]| in double (exact for fp32 operands), which equals the reference's
 * fp64 nearest-neighbour search over the same fp32 grid; on an exact tie the LOWER index wins (the reference's KD-tree leaves ties
 * unspecified).  Integer atomics only: the counts are exact and do not depend on the order of execution. */
int bg_occupancy_counts(const float* pts, int n_clouds, int P, const float* axis, int res, unsigned* point_counts,
                        unsigned* cloud_counts, bg_stream_t stream);

/* ---- evaluation clouds (sample_points.py: trimesh.sample.sample_surface on every generated STL) ------------------------------ */

/* Area-weighted surface samples of M triangle meshes in one launch (one workgroup per mesh).
 *   tri [T,3,3] fp32: the triangle soup of all meshes; tri_off [M+1] int32 (device): mesh m owns triangles tri_off[m] ..
 *   tri_off[m+1]-1, tri_off[M] = T.  cdf_ws [T] fp64 workspace.  points [M,P,3] fp32, face [M,P] int32 (triangle index WITHIN its
 *   mesh), area [M] fp64 (total surface area).
 * Per mesh: area_k = 0.5 |(b - a) x (c - a)| in fp64 (vertices widened first) and its inclusive running sum cdf_k, formed so that it
 * never decreases and a zero-area triangle repeats its predecessor's value exactly; area[m] = cdf_last.  Per point p with uniforms
 * (u0, u1, u2):  x = u0 * area[m] in fp64;  face = the smallest k with cdf_k > x (zero-area triangles are never chosen; if rounding
 * leaves no such k, the last triangle that raised the sum);  r1 = (float)u1, r2 = (float)u2, reflected (r1 = 1 - r1, r2 = 1 - r2) if
 * r1 + r2 > 1 in fp32 (trimesh's rule);  point = (a + r1 * (b - a)) + r2 * (c - a) per coordinate in fp32, every operation rounded on
 * its own (no fma).
 * uniforms [M,P,3] fp64 in [0,1), or NULL: then one Philox4x32-10 block per point, key = seed, counter = (p, low 32 bits of g, draw_id,
 * 0x5A3D0000 | bits 32..47 of g) with g = first_mesh + m the GLOBAL mesh index;  u0 = (k + 0.5) * 2^-52 with k the top 52 bits of
 * (word0 << 32 | word1) -- exact in fp64, never 0 or 1 --, u1 / u2 = ((word >> 9) + 0.5) * 2^-23 of words 2 / 3.  A cloud depends only
 * on (seed, draw_id, g, the mesh): a rank that owns meshes [lo, hi) passes first_mesh = lo and reproduces those clouds bit for bit.
 * A mesh without triangles, or whose area is not finite and positive, gets area[m] as computed, face = -1 and NaN points.
 * Device pointers, asynchronous, no allocation; M == 0 returns 0. */
int bg_mesh_sample(const float* tri, const int* tri_off, int M, int P, unsigned long long seed, unsigned draw_id, long long first_mesh,
                   const double* uniforms, double* cdf_ws, float* points, int* face, double* area, bg_stream_t stream);

/* ---- full VAEs (trainer.py:11-264: SurfVAETrainer / EdgeVAETrainer train and validate the auto-encoders whose checkpoints the
 * decoders above load) ------------------------------------------------------------------------------------------------------- */

/* diffusers' DiagonalGaussianDistribution on the encoder's moments (network.py:513-514), as the two VAE trainers use it between
 * `encode` and `decode` (trainer.py:79-84, 118-119, 206-214, 248-249): sample the posterior and its KL to N(0, I) in one launch.
 *   moments [n, P, 2L] fp32 channels-last (what the encode programs write): channels 0 .. L-1 the mean, L .. 2L-1 the log-variance.
 *   lv = clamp(logvar, -30, 20);  std = expf(0.5f * lv);  z = mean + std * eps  (fp32, the product and the sum rounded separately);
 *   kl[b] = 0.5 * sum over the P * L elements of sample b of (mean^2 + exp(lv) - 1 - lv): every term formed in fp64 from the fp32
 *   inputs (as mean^2 + (expm1(lv) - lv)), summed in fp64 in an order fixed by P * L alone, rounded to fp32 once.  No atomics: a
 *   sample's z, lv and kl are the same bits in any batch and any call.
 * noise [n, L, P] fp32 (the reference's N,C,... order: what randn(mean.shape) gives), or NULL: then element e = c * P + p of sample b
 * is exactly what bg_philox_randn gives for (seed, draw_id, first_sample + b, e) with per_sample = P * L -- a rank that owns samples
 * [lo, hi) passes first_sample = lo and reproduces those rows of the single-GPU draw.
 * z_out [n, P, L] channels-last (what the decode programs take); logvar_out [n, P, L] (optional): the CLAMPED log-variance;
 * kl_out [n] (optional).  Any P * L >= 1 that fits an int.  n == 0 returns 0 without a launch. */
int bg_vae_posterior(const float* moments, const float* noise, long long n, int P, int L, unsigned long long seed, unsigned draw_id,
                     long long first_sample, float* z_out, float* logvar_out, float* kl_out, bg_stream_t stream);

/* ---- training batches (dataset.py: filter_data / load_data, SurfPosData .. EdgeZData.__getitem__, SurfData / EdgeData; utils.py
 * pad_repeat, pad_zero, rotate_axis, get_bbox, rotate_point_cloud) ------------------------------------------------------------- */

/* N records packed once on the device (a HOST struct of device pointers).  Record r owns faces face_off[r] .. face_off[r+1]-1 and edges
 * edge_off[r] .. edge_off[r+1]-1; GLOBAL face g owns adj_idx[adj_off[g] .. adj_off[g+1]-1], the pickles' faceEdge_adj: edge ids LOCAL
 * to the record.  surf_ncs / edge_ncs 16-byte aligned. */
typedef struct bg_cad_store {
    const float* surf_ncs;      /* [n_faces, 32, 32, 3] */
    const float* surf_pos;      /* [n_faces, 6]      surf_bbox_wcs */
    const float* edge_ncs;      /* [n_edges, 32, 3] */
    const float* edge_pos;      /* [n_edges, 6]      edge_bbox_wcs */
    const float* corner_wcs;    /* [n_edges, 2, 3] */
    const int* face_off;        /* [n_records + 1] */
    const int* edge_off;        /* [n_records + 1] */
    const int* adj_off;         /* [n_faces + 1] */
    const int* adj_idx;         /* [n_adj] */
    int n_records, n_faces, n_edges, n_adj;
} bg_cad_store;

/* Recorded draws that replace the device's Philox draws in the plan (all device pointers; a NULL member reads as u = 0, turns = 1, keys
 * = 0, i.e. not augmented / the identity permutation).  Key arrays are indexed by the source face's LOCAL index and the position in its
 * adjacency list; only the first F (or degree) entries of the *1 arrays are read, all max_face (max_edge) entries of the *2 arrays, and
 * those only where there is a second shuffle (face_key2: SurfPos, edge_key2: EdgePos).  To replay a permutation p (out[i] = in[p[i]])
 * pass key[p[i]] = i. */
typedef struct bg_batch_draws {
    const double* u;            /* [B]       augment iff aug && u > 0.5 */
    const int* turns;           /* [B, 3]    quarter turns about x, y, z, each in 1 .. 3 */
    const uint32_t* face_key1;  /* [B, S] */
    const uint32_t* face_key2;  /* [B, S] */
    const uint32_t* edge_key1;  /* [B, S, E] */
    const uint32_t* edge_key2;  /* [B, S, E] */
} bg_batch_draws;

/* Output tensors of a batch; only the members of the kind are read (see the gather entry below). */
typedef struct bg_batch_out {
    float* surf_pos;            /* [B, S, 6] */
    float* surf_ncs;            /* [B, S, 32, 32, 3] */
    uint8_t* surf_mask;         /* [B, S]        1 = padding */
    float* edge_pos;            /* [B, S, E, 6] */
    float* edge_ncs;            /* [B, S, E, 32, 3] */
    uint8_t* edge_mask;         /* [B, S, E]     1 = padding */
    float* vertex_pos;          /* [B, S, E, 6] */
} bg_batch_out;

/* dataset.py:22-81 filter_data for all records, one workgroup each: keep[r] = 0 iff the record has more than max_face faces, a face
 * with more than max_edge or with 0 edges, two face boxes that are "the same", or two edge boxes in one face's adjacency list that are
 * "the same"; a and b are the same iff |fp32(a_k * scale) - fp32(b_k * scale)| < (float)threshold in fp32 for all six k (numpy compares
 * the fp32 array with the Python float that way; a NaN is never the same).  The reference's greedy non_repeat loop rejects exactly when
 * ANY pair i < j is the same, so this is an all-pairs test without order dependence.  A record whose adjacency refers outside the
 * record is not kept.  keep [n_records] uint8; n_records == 0 returns 0 without a launch. */
int bg_cad_filter(const bg_cad_store* store, int max_face, int max_edge, float scale, double threshold, uint8_t* keep,
                  bg_stream_t stream);

/* The slot maps of one batch, one workgroup per CAD.  idx [B] int32 (device): GLOBAL record numbers; kind = BG_SURFPOS .. BG_EDGEZ;
 * S = max_face <= 512, E = max_edge, S * E <= 4096.
 *   face_src [B, S] int32: row of the store's face arrays that slot s copies, -1 = zero padding;
 *   edge_src [B, S, E] int32 (edge kinds): row of the edge arrays, -1 = zero padding;
 *   rot [B] int32: 0 = not augmented, else qx | qy << 2 | qz << 4 with the quarter turns about x, y, z in 1 .. 3;
 *   scale [B, 3] fp64: max |.| over the CAD's surf_pos, edge_pos, corner_wcs (an fp32 max-abs, exact, widened).
 * A permutation is the stable argsort of uint32 keys (out[i] = in[argsort(key)[i]]); pad_repeat(n -> L): r = L div n, sep = L - r n,
 * slot i < sep (r + 1) takes source i div (r + 1), any other slot sep + (i - sep (r + 1)) div r.
 *   SurfPos: faces shuffle -> pad_repeat(S) -> second shuffle over the S slots.
 *   SurfZ:   faces shuffle -> pad_zero.
 *   EdgePos: per face (original order) edges shuffle -> pad_repeat(E) -> second shuffle; faces shuffle -> pad_zero (all -1 rows).
 *   EdgeZ:   per face edges shuffle -> pad_zero; faces shuffle -> pad_zero.
 * draws == NULL: Philox4x32-10, key = seed, counter = (element, record number, draw_id, 0xDA7A0000 | tag) with tag = 0 and element =
 * local face i for the face keys (word 0 = key 1, word 1 = key 2), tag = f + 1 and element = adjacency position j for the edge keys
 * of local face f, tag = 0 and element = 0xFFFFFFFF for the CAD's own block: u = ((word0 >> 9) + 0.5) * 2^-23, turn k = 1 +
 * ((word_(1+k) * 3) >> 32).  Nothing depends on the position in the batch: a record's slice is the same in any batch.
 * A record with more than S faces or a degree above E is cut to fit and one outside the store gives all -1 (the caller checks on the
 * host; the kernel only stays in bounds).  B == 0 returns 0. */
int bg_batch_plan(const bg_cad_store* store, const int* idx, int B, int kind, int max_face, int max_edge, int aug,
                  unsigned long long seed, unsigned draw_id, const bg_batch_draws* draws, int* face_src, int* edge_src, int* rot,
                  double* scale, bg_stream_t stream);

/* The batch tensors of `kind` from a plan, one launch; EVERY element of every output of the kind is written (padding +0.0, masks 0 / 1):
 *   SurfPos: surf_pos.  SurfZ: surf_pos, surf_ncs, surf_mask.  EdgePos: edge_pos, surf_ncs, surf_pos, surf_mask.
 *   EdgeZ: edge_ncs, edge_pos, edge_mask, surf_ncs, surf_pos, vertex_pos.
 * rot[b] == 0: grids are bitwise copies; boxes and corners are x * bbox_scaled in fp32; each edge's corner pair is ordered
 * lexicographically by (x, y, z) on those values (np.lexsort; a full tie keeps the order).
 * rot[b] != 0: the composed rotation is applied as the signed coordinate permutation it is (a negated zero becomes +0.0).  Grids:
 * rotated only.  Boxes: both corners rotated, divided by the CAD's scale of that array in fp64, per-axis min / max, times bbox_scaled
 * in fp64, rounded to fp32 once.  Corners: rotated, / scale, * bbox_scaled in fp64, the pair ordered on the fp64 values, rounded once.
 * Source rows outside the store count as padding. */
int bg_batch_gather(const bg_cad_store* store, int kind, int B, int max_face, int max_edge, float bbox_scaled, const int* face_src,
                    const int* edge_src, const int* rot, const double* scale, const bg_batch_out* out, bg_stream_t stream);

/* utils.py:210-258 rotate_point_cloud as SurfData / EdgeData apply it (dataset.py:157-163, 204-211): x, out [M, P, 3] fp32, P <= 1024,
 * one wave per item.  Item m is augmented iff aug && u > 0.5; then for the axes x, y, z in turn: subtract the mean point, rotate by the
 * axis' quarter turn (a signed permutation), add the mean back, divide by the max-abs of the result -- all in fp64 (sums: per lane over
 * its points p = lane, lane + 64, .. in order, then a butterfly across the wave; fixed by P alone), rounded to fp32 once at the end.
 * Items that are not augmented are bitwise copies.  u [M] fp64 and turns [M, 3] int32 (device) replace the Philox draw: counter =
 * (0, low 32 bits of g, draw_id, 0xDA7B0000 | bits 32..47 of g) with g = first_item + m, u and the turns from the four words as in
 * the plan entry above.  M == 0 returns 0. */
int bg_points_rotate_normalize(const float* x, long long M, int P, int aug, unsigned long long seed, unsigned draw_id,
                               long long first_item, const double* u, const int* turns, float* out, bg_stream_t stream);

/* ---- training-set de-duplication (data_process/deduplicate_cad.py, deduplicate_surfedge.py; csrc/hash_dedup.hip) ----
 *
 * digest[m] = sha256(real2bit(x[m], n_bits).reshape(-1, 3).tobytes()) for the M items x [M, P, 3] fp32, 1 <= P <= 1024 points each
 * (1024: a surface grid, 32: an edge), 1 <= n_bits <= 16 (2^n - 1 is exact in fp32; the reference's default is 6).  Quantisation is
 * convert_utils.real2bit step by step in fp32, one rounding each: t = x + 1; t = t * (2^n - 1); t = t / 2; clip to [0, 2^n - 1];
 * truncate toward zero.  +-inf, -0.0 and values outside [-1, 1] follow from the clip; a NaN quantises to 0 (numpy's cast of a NaN is
 * platform-defined).  The message is the 24 P bytes of the little-endian int64 values in memory order and is never materialised.
 * digest [M, 32] uint8: the standard big-endian output bytes, so bytes(digest[m]).hex() is the reference's hexdigest.  Exactly
 * [M, 32] bytes are written.  x 4-byte aligned (16-byte loads are used where P % 4 == 0 and x is 16-byte aligned), digest 16-byte
 * aligned.  Sizes outside the limits: BG_E_SHAPE.  M == 0 returns 0. */
int bg_points_sha256(const float* x, long long M, int P, int n_bits, uint8_t* digest, bg_stream_t stream);

/* key[n] = sha256 of the concatenation of the digests off[n] .. off[n + 1] - 1 of digest [*, 32], sorted bytewise (equal digests
 * stay as many as they are): hashlib.sha256(b''.join(sorted(d))).digest().  Equal keys <=> equal sorted digest lists <=> equal
 * '_'-joined sorted hex strings of deduplicate_cad.py, up to SHA-256 collisions.  An empty group gives sha256(b'').  off [N + 1] int32
 * ascending (device), max_group = the largest group as the host knows it, at most 4096 (more: BG_E_SHAPE, nothing is launched); a
 * group that is longer after all is cut to max_group.  One workgroup per group, 32 max_group bytes of LDS.  digest and key 16-byte
 * aligned.  N == 0 returns 0. */
int bg_digest_group_keys(const uint8_t* digest, const int* off, int N, int max_group, uint8_t* key, bg_stream_t stream);

/* keep[i] = 1 iff no j < i has key[j] == key[i] on all 32 bytes, else 0, for key [N, 32] uint8 (16-byte aligned), N <= 2^30 - 1.
 * table [T] int32 is caller-owned workspace: T a power of two, T >= 2 N, T >= 2 (else BG_E_SHAPE); the entry fills it with -1 itself.
 * It is an open-addressing table of item indices: the home slot of a key is its first 8 bytes read as a little-endian integer, masked
 * to T - 1; probing is linear (slot + 1, wrapping).  Launch one claims a slot per distinct key (atomicCAS) and lowers its index
 * (atomicMin); launch two looks every key up again.  The slot a key ends in may differ from run to run, keep does not.
 * N == 0 returns 0. */
int bg_first_occurrence(const uint8_t* key, long long N, int* table, long long T, uint8_t* keep, bg_stream_t stream);

/* ---- the update half of a trainer iteration (trainer.py: clip_grad_norm_, GradScaler.step / update, torch.optim.AdamW; csrc/optim.hip) ----
 *
 * Multi-tensor kernels over a device-resident table: one row per (param, grad, exp_avg, exp_avg_sq) quadruple of fp32, contiguous,
 * 4-byte aligned tensors of numel elements each, and a chunk list that cuts every tensor into pieces of BG_OPTIM_CHUNK elements
 * (the last one short; a tensor of 0 elements has none).  Launches use min(n_chunks, BG_OPTIM_MAX_BLOCKS) workgroups of 256 threads;
 * workgroup b walks chunks b, b + grid, ...; inside a chunk thread t owns elements 4 (t + 256 j) .. + 3, j = 0 .. 3 -- a 16-byte
 * access where every pointer of the chunk is 16-byte aligned, 4-byte accesses elsewhere.  Nothing here synchronises, allocates or uses
 * atomics; every result is a function of the table, the chunk list and the data alone (bit-reproducible).  tests/optim_restate.py
 * states the arithmetic in numpy. */
#define BG_OPTIM_CHUNK 4096
#define BG_OPTIM_MAX_BLOCKS 2048
typedef struct bg_mt_row {
    float* p; const float* g; float* m; float* v;   /* device; bg_mt_grad_stats / bg_mt_scale_grads read g (and numel) only */
    long long numel;
    double lr;                                      /* the group's learning rate, as the host holds it */
    float decay;                                    /* float(1 - lr * weight_decay), formed in double on the host */
    int has_decay;                                  /* 0: weight_decay == 0, the multiplication is skipped */
} bg_mt_row;
typedef struct bg_mt_chunk { long long first; int tensor; int _pad; } bg_mt_chunk;      /* elements first .. of row `tensor` */
typedef struct bg_optim_state {                     /* device; all zero except the powers (1.0) before the first step */
    double beta1_pow, beta2_pow;                    /* beta^step, one fp64 multiplication per successful step */
    int step;                                       /* successful steps so far */
    float total_norm;                               /* of the last finish */
    int found_inf;                                  /* of the last finish */
    int _pad;
} bg_optim_state;
typedef struct bg_scaler_state { float scale; int growth_tracker; } bg_scaler_state;      /* device; torch.amp.GradScaler's two tensors */

/* Launch 1.  partials: BG_OPTIM_MAX_BLOCKS x 16 bytes of caller-owned device memory, 16-byte aligned; workgroup b writes entry b =
 * (fp64 sum of double(g) * double(g) over its chunks, bits of the largest finite |g|, 1 if any g is inf or NaN).  Per thread the
 * elements are added in the order chunk, j, element; then a 64-lane butterfly (xor 32, 16, .. 1), then ((w0 + w1) + w2) + w3 over
 * the four waves.  n_chunks == 0 returns 0 and launches nothing. */
int bg_mt_grad_stats(const bg_mt_row* table, const bg_mt_chunk* chunks, int n_chunks, void* partials, bg_stream_t stream);

/* Launch 2.  Every workgroup sums the partials (lane l of one wave adds entries l, l + 64, .. in order, then the butterfly) and forms
 *   total_norm = float(sqrt(sum));  c = max_norm >= 0 ? min(1, max_norm / (total_norm + 1e-6f)) : 1   (fp32; max_norm < 0: no clipping)
 *   r = scaler ? float(1.0 / double(scaler->scale)) : 1;  found_inf = any non-finite g, or fl(fl(maxabs * c) * r) not finite.
 * found_inf: returns, no byte of any p, m, v is written.  Otherwise per element, fp32, one rounding per operation, with
 * bc_i = 1 - state->beta_i_pow * beta_i (fp64):
 *   g' = (g * c) * r;  p = p * decay (has_decay only);  m = m + (g' - m) * float(1 - beta1);  v = v * float(beta2) + float(1 - beta2) * (g' * g');
 *   denom = sqrt(v) / float(sqrt(bc2)) + float(eps);  p = p - float(lr / bc1) * (m / denom).
 * g is read only; state and scaler are read only (bg_optim_finish advances them).  scaler may be NULL. */
int bg_mt_adamw_step(const bg_mt_row* table, const bg_mt_chunk* chunks, int n_chunks, const void* partials, const bg_optim_state* state,
                     const bg_scaler_state* scaler, float max_norm, double beta1, double beta2, double eps, bg_stream_t stream);

/* Launch 3, one wave.  Derives total_norm and found_inf as launch 2 did (same max_norm, same scaler state) and publishes them in
 * state.  found_inf: scale *= backoff_factor, growth_tracker = 0.  Otherwise step += 1 and beta_i_pow *= beta_i (n_chunks > 0 only), growth_tracker += 1, and
 * at growth_tracker == growth_interval: scale *= growth_factor if that is finite, growth_tracker = 0 (torch's _amp_update_scale_).
 * scaler may be NULL (the factors are ignored). */
int bg_optim_finish(const void* partials, int n_chunks, bg_optim_state* state, bg_scaler_state* scaler, float max_norm, double beta1,
                    double beta2, double growth_factor, double backoff_factor, int growth_interval, bg_stream_t stream);

/* g = g * c in place with c of launch 2 (max_norm >= 0) from the partials of a bg_mt_grad_stats over the same lists: the stand-alone
 * clip_grad_norm_.  norm_out (device fp32, may be NULL) receives total_norm; n_chunks == 0 writes 0 there. */
int bg_mt_scale_grads(const bg_mt_row* table, const bg_mt_chunk* chunks, int n_chunks, const void* partials, float max_norm,
                      float* norm_out, bg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
