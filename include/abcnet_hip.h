/* abcnet_hip.h -- C ABI of libabcnet_hip.so: the MI355X (gfx950) kernels behind
 * ABC-Net's U-Net hot path.
 *
 * The reference (zhang-xuan1314/ABC-Net) has NO native interface: every FLOP of
 * the path runs inside torch ops.  Each entry point
 * below therefore names the reference *torch call site* it replaces (file:line
 * under /root/reference).  The binding a maintainer adds is the ctypes stub in
 * INTEGRATION.md; abc-net_amd/_lib.py is that stub in full.
 *
 * Conventions
 *  - plain pointers and sizes only: device pointers are raw HBM addresses owned by
 *    the caller (torch tensors stay owned by torch); nothing is retained past a call;
 *  - every function enqueues on the given hipStream_t, never allocates, never
 *    synchronises (graph-capture safe), and returns 0 on success or a negative
 *    abc_status (abc_last_error() gives text); no exceptions cross the boundary;
 *  - activations are NHWC with an explicit pixel stride (ld*, in elements) and a
 *    channel offset, so concat buffers are written/read in place (unet.py:51-59);
 *  - dtype codes: 0 = float32, 1 = bfloat16.  Accumulation is always float32.
 *  - one host thread per GPU/process (mirrors mp.spawn, multi_gpu_train.py:36).
 */
#ifndef ABCNET_HIP_H
#define ABCNET_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* abc_stream_t; /* hipStream_t */

enum abc_status { ABC_OK = 0, ABC_EINVAL = -1, ABC_EUNSUPPORTED = -2, ABC_ELAUNCH = -3 };
enum abc_dtype { ABC_F32 = 0, ABC_BF16 = 1, ABC_FP8 = 2 /* OCP e4m3fn: the fp8 inference graph only (abc_conv_desc.out_scale) */ };
#define ABC_MAX_TAPS_C 49

/* A raw (pre-BatchNorm) activation tensor consumed through its BN affine +
 * activation, optional 2x2 max-pool and optional dropout, all applied ON LOAD:
 *   v = max(y, slope*y), y = scale[c]*x + shift[c]      (BN+ReLU: unet.py:13-17,
 *                                                         BN+LeakyReLU: unet.py:67-68)
 *   pool: max over the 2x2 window of v                   (nn.MaxPool2d(2): unet.py:30)
 *   dropout: v * keep/(1-p)                              (nn.Dropout(0.2): unet.py:69)
 * scale == NULL means identity.  Coefficient arrays are indexed by the absolute
 * channel inside x (so a concat buffer carries one array for both halves). */
typedef struct abc_act_src {
    const void* x;
    const float* scale;
    const float* shift;
    const float* slope;
    int32_t Hx, Wx, ldx; /* physical dims / pixel stride of x */
    int32_t pool;
    float drop_p;
    uint32_t drop_seed;
    int32_t planar;      /* 1: x is channel-planar f32 [B][ctot][Hx][Wx] (the reference's NCHW head maps and
                            their gradients, unet.py:119); ldx is ignored, no pool/dropout */
    int32_t ctot;
    const uint32_t* drop_salt; /* device scalar added to drop_seed (NULL = 0): a counter the caller bumps once per step
                                  (abc_counter_add_u32), so that a captured graph draws a fresh mask every replay, as
                                  nn.Dropout does every forward (unet.py:69) */
} abc_act_src;

/* One head's 1x1 convolution (unet.py:70) computed in the epilogue of the convolution that produces its 128 features
 * (abc_conv_desc.heads_epi; folded inference graph): w2 = the head's packed conv2 weights as abc_pack_conv_weights writes them
 * for the heads' 1x1 kernel (layout 0: bf16 [1][4 chunks][Cout_pad][32] / e4m3 [1][2 chunks][Cout_pad][64]), bias [Cout],
 * oscale [Cout] (e4m3 only: feature scale x weight-row scale), y = the head's NCHW f32 map [B][Cout][Hout][Wout]. */
typedef struct abc_heads_epi {
    const void* w2; const float* bias; const float* oscale; float* y;
    int32_t Cout, Cout_pad;
} abc_heads_epi;

/* Generic tap-list convolution as implicit GEMM on MFMA.  One descriptor covers
 *   nn.Conv2d 3x3/5x5/1x1 forward   (unet.py:12,15,66,70; unet2.py:56,59,66)
 *   its data gradient               (autograd of the same, train.py:140)
 *   nn.ConvTranspose2d(k3,s2) forward as 4 output-parity phases, written straight
 *   into the concat buffer with the crop of unet.py:51-57 folded in (unet.py:44)
 *   and its data gradient (stride-2 gather).
 * out[b, g*om+o0, cout_off+n] = bias[n] + sum_t sum_c  W[t][c][n] * in[b, g*stride + d_t, cin_off+c]
 * Weights are pre-packed by abc_pack_conv_weights as [tap][Cin/CK][Cout_pad][CK]. */
typedef struct abc_conv_desc {
    abc_act_src src;
    const void* w;
    const float* bias; /* [Cout] or NULL */
    void* y;
    float* stats;      /* NULL, or per-block partial (sum, sumsq) [nblk][2][Cout] of the f32 outputs */
    int32_t dtype_in, dtype_c, dtype_out;
    int32_t B, Hin, Win; /* logical input dims (after the optional pool) */
    int32_t cin_off, Cin; /* real channel count; padded to the K-chunk (16, or 32 for bf16 when Cin%32==0)
                             with zeros on load, so the 1-channel image (unet.py:83) goes through here too */
    int32_t Hg, Wg;       /* output grid iterated by the kernel */
    int32_t Hout, Wout, ldy, cout_off, Cout, Cout_pad;
    int32_t stride, om, oy0, ox0;
    int32_t ntaps;
    int8_t tap_dy[ABC_MAX_TAPS_C];
    int8_t tap_dx[ABC_MAX_TAPS_C];
    int32_t stats_rows;  /* 0/2: stats = [nblk][2][Cout] (sum, sumsq); 4: [nblk][4][Cout] adds (max, min) of the
                            f32 outputs per workgroup = per-image partials for CBAM's global pools (unet2.py:19-21) */
    int32_t accumulate;  /* 1: y += result (NHWC only): a second data-gradient summed into the same tensor
                            (residual branch of unet2.DoubleConv, unet2.py:72) */
    int32_t planar_out;  /* 1: y is channel-planar f32 [B][ctot_out][Hout][Wout] (NCHW logits written directly by
                            the heads' 1x1 conv: the list forward() returns needs no layout pass); ldy ignored */
    int32_t ctot_out;
    int32_t out_act;     /* 1: the epilogue stores max(v, out_slope * v) instead of v (v = result + bias): with BatchNorm folded into
                            the weights / bias (eval mode: abc_pack_desc.row_scale, abc_bn_eval_fold) the output is the ACTIVATED
                            tensor and its consumers load it with the identity transform; the statistics stay those of v */
    float out_slope;     /* 0 = ReLU, 0.01 = LeakyReLU */
    void* pool_y;        /* optional second output: nn.MaxPool2d(2) of the stored tensor (unet.py:30), NHWC [B][Hout/2][Wout/2][ld_pool],
                            same dtype as y -- saves the separate abc_pool_act pass of the folded inference graph.  Only where
                            abc_conv_variant() == 5 (the narrow-level kernel); abc_conv_fwd refuses it elsewhere */
    int32_t ld_pool;
    /* optional (narrow-level kernel, 16 input channels, 3x3): the input tensor is not read but COMPUTED on the fly as the
     * network's first convolution of the folded inference graph (unet.py:12-14, one input channel):
     *   in[p][c] = lrelu(sum_t stem_x[p + d_t] * stem_w[c][t] * stem_scale[c] + stem_bias[c]; stem_slope)
     * over the same 3x3 taps (zero padding), stem_x = the f32 image [B][Hin][Win]; src.x is ignored */
    const float* stem_x; const float* stem_w; const float* stem_scale; const float* stem_bias; float stem_slope;
    /* fp8 (e4m3) inference graph -- the 128-channel 3x3 convolutions of the BatchNorm-folded eval graph (img2smiles2.py:42-59;
     * SURVEY.md section 8f.4) on the block-scaled MFMA with unit scales (2 x the bf16 rate):
     *   dtype_c = ABC_FP8 (then dtype_in = ABC_FP8 too): x and the packed weights are e4m3, x = real value / s_in (per tensor),
     *   w = real (BatchNorm-folded) weight / s_w[n] (per output row); out_scale[n] = s_in * s_w[n] turns the f32 accumulator back:
     *   v = acc * out_scale[n] + bias[n], then the activation (out_act).
     *   dtype_out = ABC_FP8 (with bf16 or fp8 compute): the stored value is v * (*out_quant) rounded to e4m3 (saturating at 448),
     *   *out_quant = 1 / s_out, a DEVICE scalar (calibrated per tensor: abc_fp8_act_scale), read by the kernel.
     * Served by the weights-direct loop of the lean kernel only (3x3, stride 1, Cout a multiple of 128, Cin a multiple of 64). */
    const float* out_scale;
    const float* out_quant;
    int32_t out_quant_stride; /* 0: one scalar; 1: one value per 128-channel block of the output (out_quant[n / 128]): the eight heads'
                                 features side by side in one tensor, each head with its own scale */
    const abc_heads_epi* heads_epi; /* NULL, or a DEVICE array of Cout / 128 entries: every 128-channel block of this convolution's output is
                                 one head's finished feature slice (out_act set, BatchNorm folded) and the head's 1x1 convolution is computed
                                 in the tile's epilogue -- y is not written at all, the heads' maps are.  3x3, stride 1, bf16 or e4m3 compute,
                                 the weights-direct tile (abc_conv_variant == 1); abc_conv_fwd refuses it elsewhere */
    /* act_bwd in the epilogue (training's data gradients): NULL, or the raw convolution output y_raw [B, Hout, Wout, actbwd_ld] (bf16) of the
     * layer whose ACTIVATION OUTPUT this convolution differentiates (autograd of unet.py:12-17 under train.py:140).  The kernel then stores
     *   g = dA * (BatchNorm(y_raw) > 0 ? 1 : slope),   BatchNorm(y_raw) = actbwd_scale * y_raw + actbwd_shift,
     * instead of dA, and writes that layer's BatchNorm-backward partial sums to `stats` (stats_rows = 2; abc_conv_stat_blocks rows of
     * [2][Cout]: sum of g, sum of g * (y_raw - actbwd_mean) * actbwd_invstd) -- exactly what abc_act_bwd computes from dA in a pass of its
     * own (abc_act_bwd_desc: y_raw, scale, shift, slope, mean, invstd, partial), so abc_bn_finalize_bwd consumes them unchanged.
     * Served where abc_conv_actbwd_ok() says so (bf16, stride 1: whole tiles of the lean kernel, any shape of the 16-channel narrow-level
     * kernel); abc_conv_fwd refuses it elsewhere. */
    const void* actbwd_y;
    int32_t actbwd_ld, actbwd_coff;        /* y_raw's row length and first channel (elements) */
    const float *actbwd_scale, *actbwd_shift, *actbwd_slope, *actbwd_mean, *actbwd_invstd;   /* per output channel of THIS convolution */
    /* The peak-NMS outputs of img2smiles2.py:61-79 straight from the heads' 1x1 kernel (abc_conv_variant == 3 only; abc_conv_fwd and
     * abc_heads_batch refuse it elsewhere): head_aux = a second NCHW f32 output [B][Cout][Hout][Wout] holding
     *   head_aux_mode 1: |v|                                        (img2smiles2.py:73, the rho head)
     *   head_aux_mode 2: 1.0 where v >= both circular neighbours along the CHANNEL axis and v > -1, else 0.0
     *                    (img2smiles2.py:75-79, the omega head: Cout <= 64)
     * of the value v this launch stores to y -- the lane that computed v holds its channel neighbours (or gets them by one
     * cross-lane exchange), so the maps are not read back (abc_nms_peaks with n_omega = 0 then does the two 3x3 spatial masks
     * alone).  With head_aux set, y may be NULL: the raw map is then not stored.
     *   head_aux_mode 3: head_aux is a UINT8 map [B][Cout / 6][Hout][Wout] = arg max over g = 0..5 of channel g * (Cout / 6) + bin
     *                    (first maximum, as torch.argmax: img2smiles2.py:71,112 -- bond_types_pred.view(-1, 6, 60, H, W), .argmax(0) --
     *                    the only use the decoder makes of the 360-channel bond-type head); y must be NULL, Cout / 6 <= 64, no dropout.
     *                    abc_extract_desc.btype_idx consumes it. */
    float* head_aux;
    int32_t head_aux_mode;
} abc_conv_desc;

/* number of per-block stat partials abc_conv_fwd writes for this descriptor */
int abc_conv_stat_blocks(const abc_conv_desc* d);
/* n convolutions (an array of descriptors) issued as ONE launch where they share a tile geometry of the lean kernel -- the four
 * output-parity phases of nn.ConvTranspose2d(k3, s2) (unet.py:44: four 1 / 2 / 2 / 4-tap convolutions of the same input into
 * interleaved output pixels) -- and one after the other otherwise: the result is that of n abc_conv_fwd calls either way.
 * abc_conv_batch_ok tells which of the two it will be (1: one launch). */
int abc_conv_fwd_batch(const abc_conv_desc* d, int32_t n, abc_stream_t stream);

/* nn.ConvTranspose2d(Cin -> Cout, kernel 3, stride 2) + the crop of the first output row and column that unet.py:51-56 applies when the
 * skip tensor has 2n rows / columns (every level when the input size is a multiple of 32), forward, bias included: all four output-parity
 * phases in ONE pass over the input (convt_fused.hip) -- the same result as the four abc_conv_fwd phase calls (engine.convT_phase_taps).
 *   src          the input, NHWC bf16, with the producer's BatchNorm + activation applied on load (abc_act_src; no pool / dropout / planar)
 *   w            the NINE packed weight slices of the four phases one after the other -- phase (0,0): 1 tap, (0,1): 2, (1,0): 2, (1,1): 4,
 *                each packed by abc_pack_conv_weights mode 2 with layout 1 into [taps][Cin / 32][Cout_pad][32] -- i.e. phase p starts
 *                at slice {0, 1, 3, 5}[p] of one [9][Cin / 32][Cout_pad][32] buffer
 *   y            NHWC bf16 [B][Hout][Wout][ldy], written at channels [cout_off, cout_off + Cout); Hout = 2 Hin, Wout = 2 Win
 * abc_convt_fused_ok: 1 when the kernel serves the descriptor (bf16, both axes cropped, Cin % 32 == 0, Cout_pad % 64 == 0, Cout % 8 == 0). */
typedef struct abc_convt_desc {
    abc_act_src src;
    const void* w; const float* bias; void* y;
    int32_t dtype;                     /* ABC_BF16 */
    int32_t B, Hin, Win, cin_off, Cin;
    int32_t Hout, Wout, ldy, cout_off, Cout, Cout_pad;
} abc_convt_desc;
int abc_convt_fused_ok(const abc_convt_desc* d);
int abc_convt_fused_fwd(const abc_convt_desc* d, abc_stream_t stream);
int abc_conv_batch_ok(const abc_conv_desc* d, int32_t n);
/* 1 when abc_conv_fwd honours d->actbwd_* for this descriptor (fill everything first, `stats` included), else 0: the caller then clears
 * actbwd_y and runs abc_act_bwd as a pass of its own (the engine's fallback; same results up to the rounding of dA to bf16) */
int abc_conv_actbwd_ok(const abc_conv_desc* d);
/* which kernel abc_conv_fwd runs for this descriptor: 0 = general implicit GEMM (pool / dropout / planar / ragged
 * inputs), 1 = lean 4-wave kernel for plain NHWC inputs, 2 = one-channel first layer, 3 = heads' 1x1 into NCHW f32, 4 = its data gradient from NCHW f32.  Labels only. */
int abc_conv_variant(const abc_conv_desc* d);
int abc_conv_fwd(const abc_conv_desc* d, abc_stream_t stream);
/* tile the launcher picks for this descriptor: BN output channels x (2*mt x 16) pixels per workgroup, K-chunk ck */
int abc_conv_tile(const abc_conv_desc* d, int32_t* bn, int32_t* mt, int32_t* ck);
/* the five queries in one, for a plan that needs them all: info[7] = {abc_conv_variant, abc_conv_weight_layout, abc_conv_stat_blocks,
 * bn, mt, ck, abc_conv_actbwd_ok}; returns what abc_conv_tile returns (and like it leaves bn, mt, ck alone where that is not 0).  Fill
 * everything first, `stats` included (a placeholder will do: the answers read whether it is NULL).  Host only */
int abc_conv_route_info(const abc_conv_desc* d, int32_t* info);

/* channels per K-chunk used by the packed weight layout for (compute dtype, Cin) */
int abc_conv_chunk(int dtype_c, int Cin);

/* Repack master f32 weights into the layout abc_conv_fwd / abc_wgrad consume.
 *   mode 0: Conv2d weight [Cout][Cin][kh][kw] -> forward packing   (taps = kh*kw)
 *   mode 1: Conv2d weight -> data-gradient packing (roles of Cin/Cout swapped, taps mirrored)
 *   mode 2: ConvTranspose2d weight [Cin][Cout][3][3] -> one forward parity phase (py,px)
 *   mode 3: ConvTranspose2d weight -> data-gradient packing (stride-2 gather, 9 taps)
 * Rows beyond the real channel counts are zero.  dst element type = dtype_c. */
typedef struct abc_pack_desc {
    const float* w; void* dst;
    int32_t mode, dtype_c, Cout, Cin, kh, kw, py, px;
    int32_t rows_pad;  /* padded row count of dst (Cout_pad of the consuming conv) */
    int32_t red_pad;   /* padded reduction-channel count of THIS weight (multiple of CK) */
    int32_t red_total; /* reduction-channel count of the whole dst (>= red_off + red_pad): several weights
                          may be packed side by side along the reduction axis (the 8 heads' conv1 data
                          gradient is ONE conv over the concatenated 8x128 channels) */
    int32_t red_off;   /* where this weight's reduction channels start in dst (multiple of CK) */
    int32_t ck;        /* K-chunk of dst: abc_conv_chunk(dtype_c, red_total) */
    int32_t rows_total; /* 0, or the row count of the whole dst (>= rows_off + rows_pad): several weights may be packed one
                          below the other along the ROW (output-channel) axis -- the 8 heads' conv1 (unet.py:66,116-118) run
                          as ONE 128 -> 8 x 128 convolution over the shared trunk activation */
    int32_t rows_off;  /* where this weight's rows start in dst */
    int32_t layout;    /* 0: rows of CK elements, [tap][chunk][row][CK].  1 (bf16, CK = 32 only; abc_conv_weight_layout() says which
                          convolution wants it): inside every block of 32 rows x 64 bytes the bytes are ordered
                          [kk = 16-byte half of a lane's 32 bytes][h = lane half][r = row][16 bytes], so that ONE fragment load of
                          the weights-direct conv loop (64 lanes x 16 bytes) reads 1 KB of consecutive bytes = 8 whole cache
                          lines instead of touching 16 */
    const float* row_scale; /* NULL, or one factor per output row (modes 0 and 2: per output channel): eval-mode BatchNorm folded
                               into the convolution in front of it, w'[n][..] = w[n][..] * gamma[n] / sqrt(running_var[n] + eps) */
} abc_pack_desc;
int abc_pack_conv_weights(const abc_pack_desc* d, abc_stream_t stream);
/* abc_pack_desc.layout the kernel that serves this convolution reads its weights in */
int abc_conv_weight_layout(const abc_conv_desc* d);
/* batched form: the caller builds a table of abc_pack_item_bytes()-sized entries with abc_pack_item_fill (host
 * memory, `first` = running element offset), copies it to the device once, and packs all weights of a step in ONE launch */
int abc_pack_item_bytes(void);
int64_t abc_pack_item_fill(void* item, const abc_pack_desc* d, int64_t first);
int abc_pack_batch(const void* items_dev, int32_t nitems, int64_t total, abc_stream_t stream);

/* fp8 inference graph, calibration and weight scales (all results stay on the device: no host sync, graph-safe).
 *   abc_absmax:            *out = max(*out, max |x[i]|) over n elements of dtype (f32 / bf16); zero *out first (abc_fill_f32)
 *   abc_fp8_act_scale:     s = max(*amax, 1e-12) * margin / 448, *s_out = s, *inv_s_out = 1 / s   (per-tensor activation scale)
 *   abc_fp8_weight_scales: per output row n of a Conv2d weight [rows][K] (K = Cin * kh * kw) whose BatchNorm fold factor is
 *                          fold[n] (NULL = 1):  s_w = max_k |w[n][k] * fold[n]| / 448 (1 when the row is zero),
 *                          qmul[n] = fold[n] / s_w  (abc_pack_desc.row_scale of the fp8 packing),
 *                          deq[n] = s_w * (*s_in)   (abc_conv_desc.out_scale) */
int abc_absmax(const void* x, int32_t dtype, int64_t n, float* out, abc_stream_t stream);
/* the same over the columns [c_off, c_off + C) of an [npix][ld] tensor (C, ld, c_off multiples of 8) */
int abc_absmax_cols(const void* x, int32_t dtype, int64_t npix, int32_t ld, int32_t c_off, int32_t C, float* out, abc_stream_t stream);
int abc_fp8_act_scale(const float* amax, float margin, float* s_out, float* inv_s_out, abc_stream_t stream);
int abc_fp8_weight_scales(const float* w, int32_t rows, int32_t K, const float* fold, const float* s_in, float* qmul, float* deq,
                          abc_stream_t stream);

/* BatchNorm2d, training mode (unet.py:13,16,67): reduce the conv's stat partials
 * in f64, write the on-load coefficients (scale, shift) for consumers, keep
 * (mean, invstd) for backward, update running stats with momentum 0.1 / unbiased
 * variance and bump num_batches_tracked. */
typedef struct abc_bn_fwd_desc {
    const float* partial; int32_t nblk; int32_t C; double count;
    int32_t rows; /* rows per workgroup in `partial`: 0/2 or 4 (see abc_conv_desc.stats_rows) */
    const float* gamma; const float* beta;
    float* scale; float* shift; float* mean; float* invstd;
    float* running_mean; float* running_var; int64_t* num_batches_tracked;
    float eps, momentum;
} abc_bn_fwd_desc;
int abc_bn_finalize_fwd(const abc_bn_fwd_desc* d, abc_stream_t stream);
/* n <= 8 layers in one launch (the eight heads' BatchNorms, unet.py:67).  pstride > 0: the layers' stat partials are column
 * slices of ONE [nblk][rows][pstride] buffer (each descriptor's `partial` points at its first column: the heads' conv1
 * run as one convolution); 0: own buffers of width C */
int abc_bn_finalize_fwd_batch(const abc_bn_fwd_desc* descs, int32_t n, int32_t pstride, abc_stream_t stream);
/* eval mode: coefficients from running stats (model.eval(): img2smiles2.py:49) */
int abc_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                       float* scale, float* shift, int32_t C, float eps, abc_stream_t stream);

/* eval mode with the BatchNorm folded into the convolution in front of it (img2smiles2.py:49 inference graph): the per-row
 * weight factor scale[c] = gamma / sqrt(running_var + eps) (-> abc_pack_desc.row_scale) and the folded bias
 * bias_out[c] = (conv_bias[c] - running_mean[c]) * scale[c] + beta[c]; conv_bias may be NULL */
int abc_bn_eval_fold(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                     const float* conv_bias, float* scale, float* bias_out, int32_t C, float eps, abc_stream_t stream);

/* Backward of [BN -> act -> (dropout) -> (maxpool)] in two passes (autograd of
 * unet.py:13-17,30,67-69):
 *   pass 1 (abc_act_bwd): G = (dA_same + unpool(dA_pooled)) * act'(y) * dropout;
 *           per-block partials of sum(G), sum(G*xhat)
 *   abc_bn_finalize_bwd: dgamma, dbeta (into the gradient arena) and k1=mean(G), k2=mean(G*xhat)
 *   pass 2 (abc_bn_apply_bwd): dY = gamma*invstd*(G - k1 - xhat*k2)   (in place on G) */
typedef struct abc_act_bwd_desc {
    const void* y_raw; int32_t ld_y;        /* raw conv output [B,H,W,*] */
    const void* dA_same; int32_t ld_same;   /* grad wrt activated tensor at full res, or NULL */
    const void* dA_pool; int32_t ld_pool;   /* grad wrt pooled activated tensor [B,H/2,W/2,*], or NULL */
    void* g; int32_t ld_g;                  /* out [B,H,W,C] */
    float* partial;                         /* [nblk][2][C] */
    const float* scale; const float* shift; const float* slope; const float* mean; const float* invstd;
    int32_t dtype, B, H, W, C, cy_off, csame_off, cpool_off;
    float drop_p; uint32_t drop_seed; int32_t drop_ld; /* dropout index = pixel*drop_ld + cy_off + c */
    const uint32_t* drop_salt;                         /* as abc_act_src.drop_salt: the SAME counter as the forward's */
} abc_act_bwd_desc;
int abc_act_bwd_blocks(const abc_act_bwd_desc* d);
int abc_act_bwd(const abc_act_bwd_desc* d, abc_stream_t stream);
typedef struct abc_bn_bwd_desc {
    const float* partial; int32_t nblk; int32_t C; double count;
    const float* gamma; const float* invstd;
    float* dgamma; float* dbeta; float* k1; float* k2; float* gscale; /* gscale = gamma*invstd */
    /* optional (all or none): the same correction as ONE per-channel affine of (g, y_raw),
     *   dY = ca*g + cb*y_raw + cc,  ca = gscale, cb = -gscale*k2*invstd, cc = gscale*(mean*invstd*k2 - k1),
     * for consumers that apply it on load (abc_wgrad_desc.p_dual) instead of a separate abc_bn_apply_bwd pass */
    const float* mean; float* ca; float* cb; float* cc;
    /* optional device scalar: the partial sums are of g / in_scale -- a producer that could not know a global factor of
     * its gradient yet (the fused heads kernel: the loss normalisers are batch sums); folded into the sums and into ca */
    const float* in_scale;
} abc_bn_bwd_desc;
int abc_bn_finalize_bwd(const abc_bn_bwd_desc* d, abc_stream_t stream);
/* n <= 8 layers in one launch; pstride > 0: their partial sums are column slices of one [nblk][2][pstride] buffer */
int abc_bn_finalize_bwd_batch(const abc_bn_bwd_desc* descs, int32_t n, int32_t pstride, abc_stream_t stream);
typedef struct abc_bn_apply_desc {
    void* g; int32_t ld_g; const void* y_raw; int32_t ld_y; int32_t cy_off;
    const float* mean; const float* invstd; const float* k1; const float* k2; const float* gscale;
    int32_t dtype, C; int64_t npix;
    void* out; int32_t ld_out;   /* NULL: dY replaces g in place; else dY goes to out[pixel * ld_out + c] and g is kept */
} abc_bn_apply_desc;
int abc_bn_apply_bwd(const abc_bn_apply_desc* d, abc_stream_t stream);

/* Weight gradient of a tap-list convolution (autograd of unet.py:12,15,44,66,70):
 *   dW[t][a][b] = sum_p P[p][a] * Q[stride*p + d_t][b]
 * regular conv: P = dY (a = cout), Q = activated input (b = cin), stride 1
 * transposed conv: P = activated input (a = cin), Q = dOut (b = cout), stride 2
 * Two stages: split-K partial slabs, then abc_wgrad_reduce sums the slabs and
 * writes the reference layout [a][b][taps] into the f32 gradient arena. */
typedef struct abc_wgrad_desc {
    abc_act_src p;  /* un-shifted operand */
    abc_act_src q;  /* shifted operand (halo) */
    float* partial; /* [nsplit][ntaps][Ca_pad][Cb_pad] */
    int32_t dtype_p, dtype_q, dtype_c;
    int32_t B, Hg, Wg;  /* grid of p */
    int32_t Hq, Wq;     /* logical dims of q */
    int32_t cp_off, Ca, cq_off, Cb;
    int32_t stride, ntaps, nsplit;
    int8_t tap_dy[ABC_MAX_TAPS_C];
    int8_t tap_dx[ABC_MAX_TAPS_C];
    /* BatchNorm-backward correction fused into the load of P (replaces abc_bn_apply_bwd for this layer):
     * p_dual = 1: P[p][a] = p.scale[a]*p.x[p][a] + p.slope[a]*p2[p][cp2_off + a] + p.shift[a]  (no activation), where p.x is
     * the act_bwd output g and p2 the layer's raw conv output; the corrected values are also stored to p_out
     * (NHWC, pixel stride ld_pout, same dtype as p) for the data-gradient conv that runs afterwards.
     * Only where abc_wgrad_fuses_apply() says so; otherwise abc_wgrad returns ABC_EUNSUPPORTED for p_dual. */
    const void* p2; int32_t ld_p2, cp2_off, p_dual; void* p_out; int32_t ld_pout;
    /* optional, heads' 1x1 kernel only (planar f32 P): per-split row sums of the transformed P, [nsplit][Ca_pad] --
     * the bias gradient of the conv (sum over pixels of dY) falls out of the operand the kernel holds anyway;
     * reduce with abc_wgrad_reduce(ntaps = 1, Cb = Cb_pad = 1).  abc_wgrad_rowsum_ok() says whether it is written. */
    float* rowsum_partial;
} abc_wgrad_desc;
int abc_wgrad_rowsum_ok(const abc_wgrad_desc* d);
int abc_wgrad_fuses_apply(const abc_wgrad_desc* d); /* 1: this descriptor (with p_dual set) is served by the fused path */
int abc_wgrad_pads(const abc_wgrad_desc* d, int32_t* ca_pad, int32_t* cb_pad);
int abc_wgrad_tile(const abc_wgrad_desc* d, int32_t* at, int32_t* bt); /* 32x32 tile pairs per workgroup: at x bt */
/* which kernel the launch will take: info[8] = {family (0 head, 1 one-channel, 2 16-channel, 3 5x5 32-channel, 4 general), at, bt, and for
 * the general kernel (else 0): patch rows / 8 (pm), tap-split form (ts), both operands prefetched (fast), static 3x3 K-step (k3), Q's
 * segment table in LDS}.  Host only, for tests that must prove their case reaches a path */
int abc_wgrad_route_info(const abc_wgrad_desc* d, int32_t* info);
int abc_wgrad_blocks(const abc_wgrad_desc* d); /* workgroups per split: choose nsplit so that blocks*nsplit fills the GPU */
int abc_wgrad(const abc_wgrad_desc* d, abc_stream_t stream);
typedef struct abc_wgrad_reduce_desc {
    const float* partial; int32_t nsplit, ntaps, Ca, Cb, Ca_pad, Cb_pad;
    float* dw;    /* [Ca][Cb][ntaps] */
    int32_t accumulate; /* 1: add to dw instead of overwrite */
} abc_wgrad_reduce_desc;
/* the heads' 1x1 weight gradients of all heads in one launch (each descriptor with its own partial / rowsum slabs) */
int abc_wgrad_heads_batch(const abc_wgrad_desc* descs, int32_t n, abc_stream_t stream);
int abc_wgrad_reduce(const abc_wgrad_reduce_desc* d, abc_stream_t stream);
/* abc_wgrad_reduce(r) and abc_bn_finalize_bwd(f) of two DIFFERENT layers as one launch (both inputs complete, neither reads the other's
 * output): in the backward chain the finaliser is a dependent ~5 us launch and the slab reduction of the layer above is independent of it */
int abc_wgrad_reduce_bn_bwd(const abc_wgrad_reduce_desc* r, const abc_bn_bwd_desc* f, abc_stream_t stream);
/* up to 16 (small) reductions in one launch; results bit-identical to abc_wgrad_reduce item by item */
int abc_wgrad_reduce_batch(const abc_wgrad_reduce_desc* descs, int32_t n, abc_stream_t stream);

/* Per-channel column sums of an NHWC tensor (bias gradients of convs that do not
 * feed a BN: unet.py:44 up.bias, unet.py:70 conv2.bias), optional per-channel scale. */
int abc_colsum_blocks(int64_t npix);
int abc_colsum(const void* x, int32_t dtype, int64_t npix, int32_t ld, int32_t c_off, int32_t C,
               const float* chan_scale, float* work /* [abc_colsum_blocks(npix)][C] */, float* out, abc_stream_t stream);
/* The same pass with a second row of sums weighted by a one-channel f32 image w[npix]: out_sum[c] = sum x[p][c] (may be NULL),
 * out_w[c] = sum x[p][c] * w[p] -- bias and weight gradient of a 1x1 convolution over a one-channel input, i.e. autograd of
 * unet2.DoubleConv's res_conv in the first block (unet2.py:62,72,135: nn.Conv2d(1, 32, 1)) in ONE pass over d(out).
 * work: [abc_colsum_blocks(npix)][2][C] floats. */
int abc_colsum_w1(const void* x, int32_t dtype, int64_t npix, int32_t ld, int32_t c_off, int32_t C, const float* w,
                  float* work, float* out_sum, float* out_w, abc_stream_t stream);

/* Fused activation + loss + dlogits (train.py:95-137).  Logits and dlogits are the 8 NCHW f32
 * head maps of unet.forward (unet.py:119), targets the reference's NCHW tensors
 * (utils.py:254-300; rho/omega f64): one thread per pixel, every access coalesced.
 * Writes the UNNORMALISED per-term gradient d(numerator_i)/d(logit) and per-block
 * partials of the 8 numerators + 8 denominators; abc_loss_finalize reduces them,
 * forms the 8 terms, the uncertainty weighting with s (train.py:127-135), the
 * total, ds, and head_scale[i] = weight_i/denominator_i, replicated per channel into
 * chan_scale (head i at chan_off[i]) which the heads' backward applies on load. */
typedef struct abc_loss_desc {
    const float* logits[8]; float* dlogits[8];
    const float* t_atom; const float* t_types; const float* t_charges; const float* t_hs; const float* t_bond;
    const float* t_btypes; const double* t_rho; const double* t_omega;
    int32_t B, h, w;
    double* partial; /* [nblk][16] */
} abc_loss_desc;
int abc_loss_blocks(const abc_loss_desc* d);
int abc_loss_fwd_bwd(const abc_loss_desc* d, abc_stream_t stream);
typedef struct abc_loss_fin_desc {
    const double* partial; int32_t nblk;
    const float* s; float* ds;         /* [10] */
    double* out;                       /* [0]=total, [1+i]=weighted term of head i, [9+i]=raw term of head i
                                          (head order of unet.forward: atom_t, types, charges, hs, bond_t, btypes, rho, omega) */
    float* chan_scale; int32_t nchan;  /* [nchan] */
    int32_t chan_off[8]; int32_t head_c[8];
    float grad_scale;                  /* multiplies the scales (1/world for the DDP gradient mean) */
} abc_loss_fin_desc;
int abc_loss_finalize(const abc_loss_fin_desc* d, abc_stream_t stream);
/* The true gradients of a standalone loss op (abcnet_amd.loss): abc_loss_finalize leaves the dlogits of abc_loss_fwd_bwd
 * unscaled and writes head i's factor weight_i/denominator_i into chan_scale; this multiplies each of the 8 maps in place by
 * head_scale[i] x (*grad_out) and ds[0..10) by (*grad_out).  grad_out is the incoming d(out)/d(loss), read on the device (no host
 * sync; (0.5 * loss).backward() stays correct).  One launch over all maps, 16-byte accesses: every map must be 16-byte aligned. */
typedef struct abc_loss_scale_desc {
    float* dlogits[8]; int64_t n[8];   /* elements of map i (B * C_i * h * w) */
    const float* head_scale;           /* [8]: the factor of head i (abc_loss_finalize's chan_scale with chan_off[i] = i, head_c[i] = 1) */
    float* ds;                         /* [10] */
    const double* grad_out;            /* device scalar */
} abc_loss_scale_desc;
int abc_loss_scale_grads(const abc_loss_scale_desc* d, abc_stream_t stream);

/* per-channel sum over batch and pixels of a planar f32 tensor [B][C][HW], times chan_scale[c]:
 * bias gradient of the heads' 1x1 convs (unet.py:70) from the NCHW dlogits */
int abc_plane_sum_work(int32_t C); /* floats of workspace */
int abc_plane_sum(const float* x, int32_t B, int32_t C, int32_t HW, const float* chan_scale, float* work, float* out,
                  abc_stream_t stream);

/* torch.optim.Adam step over a flat f32 arena (train.py:55,141): L2 decay into the
 * gradient, bias correction from the device-side step counter. */
typedef struct abc_adam_desc {
    float* p; const float* g; float* m; float* v; int64_t n;
    int64_t* step; /* device scalar, incremented by the kernel */
    float lr, beta1, beta2, eps, weight_decay, grad_scale;
} abc_adam_desc;
int abc_adam_step(const abc_adam_desc* d, abc_stream_t stream);

/* torch.optim.Adam over ANY list of f32 device tensors in one launch (abcnet_amd.optim.Adam): a device table of segments
 * (runs of elements whose p, g, m, v are each contiguous -- a whole arena is one segment) and, by value, a table of
 * hyper-parameter classes (one per distinct (param group, step count)) with the bias corrections computed on the host.
 * Same per-element arithmetic as abc_adam_step.  Segments may come in any order; seg.first_chunk is the running sum of
 * ceil(n / abc_adam_multi_chunk()) over the segments before it, chunk_total the sum over all. */
#define ABC_ADAM_MAX_CLASSES 32
typedef struct abc_adam_seg {
    float* p; const float* g; float* m; float* v;
    int64_t n;
    int64_t first_chunk;
    int32_t cls;                       /* index into abc_adam_multi_desc.cls */
    int32_t pad_;
} abc_adam_seg;
typedef struct abc_adam_class {
    float step_size;                   /* lr / (1 - beta1^step) */
    float bc2_sqrt;                    /* sqrt(1 - beta2^step) */
    float beta1, beta2, eps, weight_decay;
    float pad_[2];
} abc_adam_class;
typedef struct abc_adam_multi_desc {
    const abc_adam_seg* segs;          /* device table [nseg] */
    int32_t nseg;
    int32_t nclass;                    /* <= ABC_ADAM_MAX_CLASSES */
    int64_t chunk_total;
    abc_adam_class cls[ABC_ADAM_MAX_CLASSES];
} abc_adam_multi_desc;
int abc_adam_multi_chunk(void);        /* elements per workgroup */
int abc_adam_multi(const abc_adam_multi_desc* d, abc_stream_t stream);

/* The heads' 1x1 convolutions (unet.py:70, out_modules[i].conv2) of ALL heads in one launch: descs[0..n) are the same
 * descriptors abc_conv_fwd would take one by one (n <= 8, same batch and map size).  which = 0: forward into the NCHW
 * f32 logits; which = 1: data gradient from the NCHW f32 dlogits.  ABC_EUNSUPPORTED when a descriptor is not served by
 * the dedicated heads kernels (then call abc_conv_fwd per head). */
int abc_heads_batch(const abc_conv_desc* descs, int32_t n, int32_t which, abc_stream_t stream);

/* The heads' second half of a TRAINING step in one pass (bf16): out_modules[i].conv2 forward (unet.py:70, 116-118), the
 * activation + loss block with d(loss)/d(logits) (train.py:95-125, as abc_loss_fwd_bwd), conv2's data gradient, the
 * backward of Dropout and LeakyReLU (unet.py:67-69) and BatchNorm-backward partial sums, for the eight heads
 * [1,14,3,2,1,360,60,60] (train.py:47).  Replaces abc_heads_batch(which = 0) + abc_loss_fwd_bwd + abc_heads_batch(which
 * = 1) + abc_act_bwd; abc_heads_fused_wgrad replaces abc_wgrad_heads_batch.  Order of a step:
 *   abc_heads_fused_pack (weights changed) -> abc_heads_fused_fwd_bwd -> abc_loss_finalize(loss_partial, abc_heads_fused_loss_blocks())
 *   -> abc_heads_fused_wgrad, abc_bn_finalize_bwd(_batch) with in_scale = chan_scale + chan_off[i] and partial = bn_partial.
 * Everything the kernel writes is the gradient of each loss term's NUMERATOR (the normalisers are batch sums): g and the
 * BatchNorm sums lack the head's factor chan_scale[chan_off[i]], which the two consumers above apply. */
typedef struct abc_heads_fused_desc {
    const void* feat; int32_t ld;       /* raw conv1 outputs of all heads, NHWC bf16 [B*h*w][ld]; head i = channels [128 i, 128 i + 128) */
    const float* scale; const float* shift; const float* slope;   /* [ld]: BatchNorm + LeakyReLU applied on load */
    const float* mean; const float* invstd;                        /* [ld]: batch statistics (for xhat) */
    float drop_p; uint32_t drop_seed; const uint32_t* drop_salt;   /* Dropout after the activation (abc_act_src) */
    const float* w2[8]; const float* b2[8];   /* conv2.weight [C_i][128], conv2.bias [C_i] (reference layout, f32) */
    void* w2_pack;                      /* abc_heads_fused_pack_bytes() bytes, written by abc_heads_fused_pack */
    float* logits[8];                   /* out: NCHW f32 [B][C_i][h][w] (unet.py:119); an entry may be NULL when nothing
                                         * downstream reads that head's logits (they are then never stored: 0.3 GB less) */
    const float* t_atom; const float* t_types; const float* t_charges; const float* t_hs; const float* t_bond;
    const float* t_btypes; const double* t_rho; const double* t_omega;   /* targets, as abc_loss_desc */
    void* dl;                           /* out: d(numerator)/d(logits), bf16, abc_heads_fused_dl_elems() elements:
                                           per head [chunk][packed rows][128 pixels] (row order: abc_heads_fused_chan_of_row);
                                           with dl_tiles the bond-type rows of tiles whose bit is clear are unspecified (below) */
    void* g;                            /* out: NHWC bf16 [B*h*w][ld]: gradient w.r.t. the BatchNorm outputs, without the head's factor */
    float* bn_partial;                  /* out: [abc_heads_fused_chunks()][2][ld]: sum g, sum g * xhat */
    double* loss_partial;               /* out: [abc_heads_fused_loss_blocks()][16], the layout abc_loss_finalize reduces */
    int32_t B, h, w;                    /* h * w a multiple of 128 */
    /* abc_heads_fused_wgrad (wgrad_work: both): */
    const float* chan_scale; int32_t chan_off[8];   /* abc_loss_finalize's factors, first channel of head i */
    float* dw2[8]; float* db2[8];       /* out: conv2.weight.grad [C_i][128], conv2.bias.grad [C_i] */
    float* wgrad_work;                  /* abc_heads_fused_wgrad_floats() floats; ALSO written by abc_heads_fused_fwd_bwd (the five
                                           small heads' weight-gradient partials), so set it for both calls */
    void* keep_mask;                    /* optional, 3 * B*h*w * 16 bytes: abc_heads_fused_fwd_bwd leaves the dropout keep bits of the three
                                           wide heads' features here and abc_heads_fused_wgrad reads them instead of hashing every
                                           element again (set it for both calls, or for neither) */
    /* optional (both or neither): abc_raster_desc.group_flags of the rasteriser that drew the target maps, and 512 zero bytes.  A wave whose
     * 32 pixels carry no target of a head reads that head's targets from the zero bytes instead of the maps (train.py:107-125 on
     * all-zero targets: identical arithmetic, no HBM traffic -- the maps hold ~62 non-zero 3x3 neighbourhoods per image) */
    const uint32_t* target_flags; const void* zero_bytes;
    /* ZERO SKIP.  A softmax head (atom types, charges, hydrogens, bond types) adds nothing to its loss and has d(logits) = 0 in a
     * softmax group all of whose targets are zero (exact for finite logits).  abc_heads_fused_fwd_bwd decides this from the targets it
     * has just loaded, per 32-row tile of a wave's 32 pixels: a tile without a target stores its logits and runs neither the loss
     * arithmetic nor the data-gradient MFMAs; a wave without a firing tile writes g = 0 and zero BatchNorm sums.
     * dl_tiles: optional (both calls or neither), abc_heads_fused_chunks() words, written by every abc_heads_fused_fwd_bwd for every
     *   chunk: bit 4 mt + w of word c is set iff row tile mt of the bond-type head fired for wave w (pixels 32 w .. 32 w + 31) of chunk c.
     *   With dl_tiles the bond-type rows of `dl` are written ONLY in tiles whose bit is set -- the 32 rows x 32 pixels of a clear bit are
     *   unspecified -- and abc_heads_fused_wgrad reads `dl` only where the bit is set.  Without it those tiles are stored as zeros.
     * no_zero_skip: 0 (a zeroed descriptor) = as above; 1 = every tile takes the full arithmetic and is stored, every used bit of
     *   dl_tiles is set (the form the skip is tested and measured against). */
    uint64_t* dl_tiles; int32_t no_zero_skip; int32_t pad_;
} abc_heads_fused_desc;
int64_t abc_heads_fused_pack_bytes(void);
int abc_heads_fused_chunks(const abc_heads_fused_desc* d);
int abc_heads_fused_loss_blocks(const abc_heads_fused_desc* d);
int64_t abc_heads_fused_dl_elems(const abc_heads_fused_desc* d);
int64_t abc_heads_fused_wgrad_floats(const abc_heads_fused_desc* d);
int abc_heads_fused_rows(int32_t head);                       /* packed rows of a head (multiple of 32) */
int abc_heads_fused_chan_of_row(int32_t head, int32_t row);   /* channel of a packed row, -1 = padding */
int abc_heads_fused_pack(const abc_heads_fused_desc* d, abc_stream_t stream);
int abc_heads_fused_fwd_bwd(const abc_heads_fused_desc* d, abc_stream_t stream);
int abc_heads_fused_wgrad(const abc_heads_fused_desc* d, abc_stream_t stream);

/* Inference NMS (img2smiles2.py:61-79) on the NCHW f32 head maps: atom/bond 3x3 peak
 * masks (logit > -1), |rho|, circular 3-tap omega peak mask; outputs NCHW f32 like the reference. */
typedef struct abc_nms_desc {
    const float* atom; const float* bond; const float* rho; const float* omega;
    int32_t B, h, w, n_omega;
    float* atom_mask; float* bond_mask; float* rho_abs; float* omega_mask;
} abc_nms_desc;
int abc_nms_peaks(const abc_nms_desc* d, abc_stream_t stream);

/* Target rasteriser (utils.py:83-228, MolecularImageDataset.__getitem__) from compact per-molecule records: zeroes the 8
 * target maps of the loss (same layouts / dtypes as abc_loss_desc) and rasterises atoms, then bonds, in record order
 * (the reference's slice assignments are order dependent).  atoms[b][i] = (x, y, type, charge, hs in {0,1} or -1);
 * bonds[b][i] = (x, y, type, omega bin, single: 1 = one direction (stereo types 4, 5), 0 = bins k and k + 30);
 * rho[b][i] float64.  x = row, y = column, inside the map.  The string parsing, vocabulary look-ups and atan of
 * utils.py:94-163 stay on the host (abcnet_amd/raster.py). */
typedef struct abc_raster_desc {
    float* t_atom; float* t_types; float* t_charges; float* t_hs; float* t_bond; float* t_btypes; double* t_rho; double* t_omega;
    int32_t B, h, w, max_atoms, max_bonds;
    const int32_t* atoms; const int32_t* n_atoms;   /* [B][max_atoms][5], [B] */
    const int32_t* bonds; const int32_t* n_bonds;   /* [B][max_bonds][5], [B] */
    const double* rho;                              /* [B][max_bonds] */
    /* Sparse use of the maps (optional; all NULL / 0 = the plain form: zero all eight maps, draw).
     *   group_flags  out, uint32 [B * h * w / 32]: bit i of word g set when head i's targets (atom 0, types 1, charges 2, hs 3, bond 4,
     *                bond types 5, rho 6, omega 7) may be non-zero somewhere in pixels [32 g, 32 g + 32) of the flattened batch -- the unit a
     *                wave of abc_heads_fused_fwd_bwd owns (abc_heads_fused_desc.target_flags); h * w a multiple of 32
     *   prev_*       device scratch of the records' shapes (atoms, bonds, rho, counts [2][B]): the records the maps currently hold.
     *   incremental  1: the maps hold exactly the drawing of prev_* (a previous call with the same buffers): ERASE those pixels instead of
     *                zeroing 23 MB per image; 0: zero everything first.  Either way prev_* <- the new records. */
    uint32_t* group_flags;
    int32_t* prev_atoms; int32_t* prev_bonds; double* prev_rho; int32_t* prev_counts;
    int32_t incremental;
} abc_raster_desc;
int abc_rasterize_targets(const abc_raster_desc* d, abc_stream_t stream);

/* Input images (utils.py:42-81, the image half of MolecularImageDataset.__getitem__, with 512 generalised to S; and
 * utils_for_test.py:21-27) from raw 8-bit renders: writes f32 {0, 1} into out[B][1][S][S].
 *   mode ABC_IMG_TRAIN: the source (src_h x src_w) resized to rows x cols like OpenCV's INTER_LINEAR on float32 (horizontal pass,
 *                       then vertical, every multiply and add rounded on its own; an axis of unchanged size is copied), placed
 *                       at (ddx, ddy) on a white S x S canvas; ink = v / 255 < 0.6f (float32); salt = h(key, 2p) < salt_thr,
 *                       pepper = h(key, 2p + 1) < pepper_thr with p = x * S + y and h(key, i) = abc_noise_hash(i, abc_noise_seed(key));
 *                       out = (ink | salt) & ~pepper.
 *                       The noise matches the reference's np.random fields in distribution, not bit for bit.
 *   mode ABC_IMG_TEST:  src_h = src_w = S, no resize / pad / noise; out = (byte <= test_max_ink), the largest byte the
 *                       reference's 1 - ((u8 / 255).astype(f32) > 0.2) maps to 1 (computed by the caller).
 * params: device int32 [B][ABC_IMG_NPARAM] (thresholds and key halves as uint32 bit patterns).  An image whose parameters
 * break the contract (rows or cols above S, negative offsets, src_h above src_max_h, src_w above src_pitch, test mode with a
 * non-S x S source) is written as NaN; params_host (optional: a host copy of the table) is checked at call time instead. */
enum abc_image_param { ABC_IMG_SRC_H = 0, ABC_IMG_SRC_W, ABC_IMG_ROWS, ABC_IMG_COLS, ABC_IMG_DDX, ABC_IMG_DDY, ABC_IMG_SALT_THR,
                       ABC_IMG_PEPPER_THR, ABC_IMG_KEY_LO, ABC_IMG_KEY_HI, ABC_IMG_NPARAM };
enum abc_image_mode { ABC_IMG_TRAIN = 0, ABC_IMG_TEST = 1 };
typedef struct abc_image_desc {
    float* out;                     /* [B][1][S][S] f32, 16-byte aligned */
    const uint8_t* src;             /* image b at src + b * src_stride, its row i at + i * src_pitch (16-byte aligned) */
    int64_t src_stride;             /* bytes between images, >= src_max_h * src_pitch, multiple of 16 */
    int32_t src_pitch;              /* bytes between rows, multiple of 16, <= 1024 */
    int32_t src_max_h;              /* rows an image slot holds, <= 1024 */
    const int32_t* params;          /* device [B][ABC_IMG_NPARAM] */
    const int32_t* params_host;     /* optional host copy of params, validated at call time (NULL: not checked) */
    int32_t B, S, mode;             /* S a multiple of 8 (one thread writes 8 consecutive pixels), 8 <= S <= 8192 */
    int32_t test_max_ink;           /* ABC_IMG_TEST: ink iff byte <= test_max_ink */
} abc_image_desc;
int abc_build_images(const abc_image_desc* d, abc_stream_t stream);

/* Raw grey scans of any size into out[B][1][S][S], f32 {0, 1} (csrc/scan.hip): the offline step the reference
 * only hints at (binarize.py: cv2.threshold(img, 0, 255, THRESH_BINARY + THRESH_OTSU)) composed with utils_for_test.py:21-27, plus
 * the crop and the fit a scan needs.  Everything is exact integer arithmetic except sigma(t) below.  For image b, src_h x src_w
 * bytes (params[b]); bytes of its slot outside them are never read into any result.
 *   histogram  h[v] = the count of byte v; N = src_h * src_w <= 2^24.
 *   threshold  for t = 0 .. 255: w0 = sum_{v <= t} h[v], s0 = sum_{v <= t} v h[v], w1 = N - w0, S = s0(255),
 *              d = S w0 - N s0 (int64, exact: |d| < 2^56); t is admissible when w0 > 0 and w1 > 0;
 *              sigma(t) = ((double)d * (double)d) / ((double)w0 * (double)w1): two multiplies and one divide, each rounded on its
 *              own, never fused.  Every input is an exact integer, so the value does not depend on the order the histogram was
 *              summed in, and IEEE float64 anywhere (numpy) gives the same bits.  thr = the SMALLEST admissible t with maximal
 *              sigma.  No admissible t (one byte value only): status ABC_SCAN_CONSTANT, a blank output.
 *              sigma is the classical between-class variance up to the constant factor N^2.  It is NOT claimed to be
 *              bit-identical to OpenCV's Otsu in near-ties: no OpenCV was at hand to check against.
 *   polarity   ABC_SCAN_DARK: ink = byte <= thr (binarize.py:5 then utils_for_test.py:22-24); ABC_SCAN_LIGHT: ink = byte > thr;
 *              ABC_SCAN_AUTO: LIGHT when 2 w0(thr) > N (the dark side is the majority), else DARK.
 *   box        y0, y1, x0, x1 of the ink pixels, inclusive; bh = y1 - y0 + 1, bw = x1 - x0 + 1.
 *   fit        never upscales.  L = S - 2 margin, m = max(bh, bw); m <= L: rows = bh, cols = bw; else rows = max(1, bh L / m),
 *              cols = max(1, bw L / m) (floor division in 64 bits); ddx = (S - rows) / 2, ddy = (S - cols) / 2.
 *   resample   destination (r, c), 0 <= r < rows, 0 <= c < cols, covers source rows y0 + floor(r bh / rows) ..
 *              y0 + ceil((r + 1) bh / rows) - 1 and columns likewise with bw, cols, x0: never empty, never outside the box.
 *              n = its ink pixels, a = its area: out = 1 iff n >= 1 and 256 n >= cover_q8 a, written at (ddx + r, ddy + c);
 *              every other canvas pixel is 0 (the launch owns the whole output).
 *   geom       int32 [B][ABC_SCAN_NGEOM] per image (abc_scan_geom order); ABC_SCAN_CONSTANT and ABC_SCAN_BAD_PARAMS rows have
 *              thr = -1 and zeros in every column but the status.
 * An image whose src_h or src_w is below 1 or above its slot (src_max_h, src_pitch) is written as NaN with ABC_SCAN_BAD_PARAMS;
 * params_host (optional: a host copy of the table) is checked at call time instead (ABC_EINVAL).
 * Five launches on the stream, in order, no parallel branch (capturable), no sync, no allocation: hist and box are the caller's
 * scratch, zeroed / reset by the sequence itself. */
enum abc_scan_param { ABC_SCAN_SRC_H = 0, ABC_SCAN_SRC_W, ABC_SCAN_NPARAM };
enum abc_scan_polarity { ABC_SCAN_DARK = 0, ABC_SCAN_LIGHT = 1, ABC_SCAN_AUTO = 2 };
enum abc_scan_status { ABC_SCAN_CONSTANT = 1, ABC_SCAN_BAD_PARAMS = 2 };
enum abc_scan_geom { ABC_SCAN_G_THR = 0, ABC_SCAN_G_INVERTED, ABC_SCAN_G_STATUS, ABC_SCAN_G_Y0, ABC_SCAN_G_X0, ABC_SCAN_G_BH,
                     ABC_SCAN_G_BW, ABC_SCAN_G_ROWS, ABC_SCAN_G_COLS, ABC_SCAN_G_DDX, ABC_SCAN_G_DDY, ABC_SCAN_G_INK, ABC_SCAN_NGEOM };
enum { ABC_SCAN_NBOX = 8 };         /* scratch words per image of abc_scan_desc.box */
typedef struct abc_scan_desc {
    float* out;                     /* [B][1][S][S] f32, 16-byte aligned */
    const uint8_t* src;             /* image b at src + b * src_stride, its row i at + i * src_pitch (16-byte aligned) */
    int64_t src_stride;             /* bytes between images, >= src_max_h * src_pitch, multiple of 16 */
    int32_t src_pitch;              /* bytes between rows, multiple of 16, <= 4096 */
    int32_t src_max_h;              /* rows an image slot holds, <= 4096 */
    const int32_t* params;          /* device [B][ABC_SCAN_NPARAM] */
    const int32_t* params_host;     /* optional host copy of params, validated at call time (NULL: not checked) */
    int32_t B, S;                   /* 1 <= B <= 65535; S a multiple of 8 (one thread writes 8 consecutive pixels), 8 <= S <= 8192 */
    int32_t margin;                 /* 0 <= 2 margin < S */
    int32_t cover_q8;               /* 0 .. 256: the ink coverage (in 1/256) a destination pixel needs; 0: any ink */
    int32_t polarity;               /* abc_scan_polarity */
    uint32_t* hist;                 /* scratch [B][256] */
    int32_t* box;                   /* scratch [B][ABC_SCAN_NBOX] */
    int32_t* geom;                  /* out [B][ABC_SCAN_NGEOM] */
} abc_scan_desc;
int abc_build_scan_images(const abc_scan_desc* d, abc_stream_t stream);
/* sizeof(abc_scan_desc), for a binding's mirror struct (as abc_molblock_desc_size) */
int abc_scan_desc_size(void);

/* abc_build_scan_images with dirt and far-off text dropped before the crop (csrc/scan.hip): connected
 * components over a coarse grid of cells, weighed by their ink; the box and the resample read ink from kept cells only.  All values
 * are integers and everything is exact.  thr, inverted and the status come from the threshold above; a pixel (y, x) with y < src_h
 * and x < src_w is ink by the polarity rule above; bytes of the slot outside the source never count.
 *   cells       cell is 8, 16, 32 or 64.  Cell (cy, cx) covers rows cy cell .. min(src_h, (cy + 1) cell) - 1 and columns likewise.
 *               The grid of image b is ch = ceil(src_h / cell) by cw = ceil(src_w / cell); the capacity grid is cap_ch =
 *               ceil(src_max_h / cell) by cap_cw = ceil(src_pitch / cell).  ink(cy, cx) = the ink pixels in the cell; a cell is
 *               occupied when ink > 0.
 *   components  the 8-connected components of the occupied cells.  A component's label is the smallest cy cap_cw + cx among its
 *               cells, its weight the sum of ink over its cells; H is the largest weight.
 *   keep rule   a component is kept iff weight >= min_ink and 256 weight >= keep_q8 H, evaluated in 64 bits (min_ink >= 0, keep_q8
 *               0 .. 256).  keep_q8 = 256 keeps the heaviest component and every component that ties with it; there is no tie-break
 *               anywhere: the result depends only on the partition and the sums.  min_ink = 0 and keep_q8 = 0 keep everything, and
 *               then out and geom are abc_build_scan_images' bit for bit.
 *   box         y0, y1, x0, x1 over the ink pixels that lie in kept cells.
 *   fit         unchanged.
 *   resample    unchanged, except that n counts only ink pixels in kept cells; the area a is unchanged.  A source box may straddle
 *               kept and dropped cells.
 *   nothing kept  (min_ink > H) status ABC_SCAN_NO_COMPONENT: a blank output; the geometry row keeps thr and inverted, carries the
 *               status and has zeros elsewhere, but ink still holds the source's count.
 *   ABC_SCAN_CONSTANT and ABC_SCAN_BAD_PARAMS images behave as above and the cleaning launches skip them.
 *   geom        layout unchanged; ink stays the thresholded source's count.
 *   stats       int32 [B][ABC_SCAN_NCLEAN] (abc_scan_clean_stat order): components, kept, ink_kept, ink_dropped, heaviest (H),
 *               occupied_cells; all zeros for an image whose status was non-zero before cleaning.
 *   labels_out  optional int32 [B][cap_ch][cap_cw]: an unoccupied cell inside the image's grid holds -1, an occupied cell its
 *               component's label; cells outside the image's grid, and every cell of a skipped image, hold -1.  Every launch
 *               writes the whole of image b's slice.
 *   keep_out    optional uint8 of the same shape: 1 is a kept occupied cell, 0 everything else.
 * Nine launches on the stream, in order, whatever the images hold: zero, histogram and threshold as above; cells (one pass over the
 * source on the histogram's grid, each cell's ink summed in LDS and stored once), union (union-find over the cells: an occupied cell
 * unions with its W, NW, N and NE neighbours, the larger root always hung under the smaller by compare-and-swap), flatten (every
 * cell to its root, its ink added to the root's weight by integer atomics), decide (H, the keep bytes, stats, labels_out, keep_out
 * and the status); then the box and the fit+write passes reading the keep bytes.  No parallel branch (capturable), no sync, no
 * allocation; scratch is the caller's, abc_scan_clean_scratch_bytes of it, 16-byte aligned, and the sequence resets all it uses: a
 * smaller image after a larger one in the same slot shows nothing stale.  Every loop that follows parents is bounded by the cells of
 * the capacity grid; parents only decrease, so a correct run cannot reach the bound; an image that does gets the status
 * ABC_SCAN_CLEAN_FAILED, a blank output, a geometry row as for nothing kept, a zero stats row, and -1 / 0 in labels_out / keep_out.
 * Every guard of abc_build_scan_images applies to d; ABC_EUNSUPPORTED: cell outside the four values; ABC_EINVAL: min_ink < 0,
 * keep_q8 outside 0 .. 256, scratch or stats NULL, scratch not 16-byte aligned, stats or labels_out not 4-byte aligned.  Nothing is
 * launched after a refusal. */
enum abc_scan_clean_status { ABC_SCAN_NO_COMPONENT = 4, ABC_SCAN_CLEAN_FAILED = 8 };      /* further abc_scan_status values */
enum abc_scan_clean_stat { ABC_SCAN_C_COMPONENTS = 0, ABC_SCAN_C_KEPT, ABC_SCAN_C_INK_KEPT, ABC_SCAN_C_INK_DROPPED,
                           ABC_SCAN_C_HEAVIEST, ABC_SCAN_C_OCCUPIED, ABC_SCAN_NCLEAN };
typedef struct abc_scan_clean_desc {
    void* scratch;                  /* abc_scan_clean_scratch_bytes(B, src_max_h, src_pitch, cell) bytes, 16-byte aligned */
    int32_t* stats;                 /* out [B][ABC_SCAN_NCLEAN] */
    int32_t* labels_out;            /* optional out [B][cap_ch][cap_cw] (NULL: not written) */
    uint8_t* keep_out;              /* optional out [B][cap_ch][cap_cw] (NULL: not written) */
    int32_t cell;                   /* 8, 16, 32 or 64 */
    int32_t min_ink;                /* >= 0 */
    int32_t keep_q8;                /* 0 .. 256 */
} abc_scan_clean_desc;
int abc_build_scan_images_clean(const abc_scan_desc* d, const abc_scan_clean_desc* q, abc_stream_t stream);
/* sizeof(abc_scan_clean_desc), for a binding's mirror struct (as abc_scan_desc_size) */
int abc_scan_clean_desc_size(void);
/* the bytes of abc_scan_clean_desc.scratch for these capacities; ABC_EINVAL (negative) when one of them is outside the limits above */
int64_t abc_scan_clean_scratch_bytes(int32_t B, int32_t src_max_h, int32_t src_pitch, int32_t cell);

/* A page scan into its drawings, one canvas each (csrc/scan.hip).  d is read as abc_build_scan_images_clean
 * reads it, with d->B the number of pages P: src, params, params_host and hist are per page; out, geom and box are per canvas, and
 * there are D = q->canvases of them (box: [D][ABC_SCAN_NBOX]).  Integers only, everything exact.  Threshold, polarity, ink, cells,
 * ink(cy, cx), the capacity grid, the fit and the resample are those above, per page.
 *   groups      two occupied cells belong together when their Chebyshev distance max(|dcy|, |dcx|) is at most reach (1 .. 4);
 *               groups are the transitive closure.  reach = 1 is the 8-connected partition above.  A group's label is the smallest
 *               cy cap_cw + cx among its cells, its weight the sum of ink over its cells; H is the largest weight of the page.
 *   keep rule   per page, in 64 bits: weight >= min_ink and 256 weight >= keep_q8 H.
 *   order       a page's kept groups in ascending label (the reading order of their first cells; labels are distinct: no tie-break).
 *               A page takes its first min(kept, max_per_page) groups; a page with more gets ABC_SCAN_SPLIT_PAGE_FULL.  Canvases are
 *               given page by page in that order without holes: first[p] = sum of taken[p'] for p' < p, taken[p] = what of the page's
 *               groups fits below D; every page that lost one to D gets ABC_SCAN_SPLIT_BATCH_FULL.
 *   canvas j    of page p and group g: the box over the ink pixels of p that lie in cells of g; the fit unchanged; the resample with
 *               n counted over the ink in cells of g only, the area a unchanged.  Its geometry row: thr and inverted of the page,
 *               status 0, box, fit and offsets as for any builder, ink = the weight of g.  A canvas j >= total[0] is blank (0.0)
 *               and its row is thr = -1, status ABC_SCAN_NO_COMPONENT, zeros elsewhere.
 *   total       int32 [2]: total[0] = the canvases written (<= D), total[1] = the kept groups of all pages (the true count).
 *   drawings    int32 [D][ABC_SCAN_NDRAWING]: page, label, weight, rank_in_page; -1, -1, 0, -1 in an unused row.
 *   pages       int32 [P][ABC_SCAN_NPAGE] (abc_scan_page_stat order): status, groups, kept (by the keep rule, before max_per_page
 *               and D), first, taken, ink_kept (the ink of the kept groups), ink_dropped (the page's ink less ink_kept),
 *               occupied_cells.  status is the page's abc_scan_status (ABC_SCAN_CONSTANT, ABC_SCAN_BAD_PARAMS; ABC_SCAN_NO_COMPONENT
 *               when min_ink > H keeps nothing; ABC_SCAN_CLEAN_FAILED when a parent walk reached its bound) or-ed with the two
 *               overflow bits.  A CONSTANT, BAD_PARAMS or CLEAN_FAILED page has no drawings and zeros in every other column but
 *               first; it owns no canvas (so no NaN is written) and disturbs no other page.
 *   labels_out  optional int32 [P][cap_ch][cap_cw]: an occupied cell's label, -1 elsewhere and on pages without drawings.
 *   canvas_out  optional int32 of the same shape: the canvas a cell's ink goes to, -1 for none.
 * Every word of out, geom, total, drawings, pages and the optional slices is written by every call.
 * Ten launches on the stream, in order, whatever the pages hold: zero, histogram, threshold, cells, union (every occupied cell
 * with the occupied cells in the preceding half of its (2 reach + 1)^2 window), flatten, rank (one workgroup per page: H, the keep
 * rule, each kept group's rank in label order, the page row), pack (one workgroup: first, taken, total, drawings, each cell's
 * canvas, the canvases' box words), box (per canvas), fit+write (per canvas).  No parallel branch (capturable), no sync, no
 * allocation; scratch is the caller's, abc_scan_split_scratch_bytes of it, 16-byte aligned, and the sequence resets all it uses.
 * Every guard of abc_build_scan_images applies (B to P); ABC_EUNSUPPORTED: cell outside 8 / 16 / 32 / 64; ABC_EINVAL: canvases
 * outside 1 .. 65535, max_per_page outside 1 .. ABC_SCAN_SPLIT_MAX_PER_PAGE, reach outside 1 .. 4, min_ink < 0, keep_q8 outside
 * 0 .. 256, a NULL scratch, pages, drawings or total, scratch not 16-byte aligned or a table not 4-byte aligned.  With params_host
 * set a bad page is refused at call time (ABC_EINVAL) as above.  Nothing is launched after a refusal. */
enum abc_scan_split_status { ABC_SCAN_SPLIT_PAGE_FULL = 16, ABC_SCAN_SPLIT_BATCH_FULL = 32 };      /* further page status bits */
enum abc_scan_page_stat { ABC_SCAN_P_STATUS = 0, ABC_SCAN_P_GROUPS, ABC_SCAN_P_KEPT, ABC_SCAN_P_FIRST, ABC_SCAN_P_TAKEN,
                          ABC_SCAN_P_INK_KEPT, ABC_SCAN_P_INK_DROPPED, ABC_SCAN_P_OCCUPIED, ABC_SCAN_NPAGE };
enum abc_scan_drawing { ABC_SCAN_D_PAGE = 0, ABC_SCAN_D_LABEL, ABC_SCAN_D_WEIGHT, ABC_SCAN_D_RANK, ABC_SCAN_NDRAWING };
enum { ABC_SCAN_SPLIT_MAX_PER_PAGE = 64, ABC_SCAN_SPLIT_MAX_REACH = 4 };
typedef struct abc_scan_split_desc {
    void* scratch;                  /* abc_scan_split_scratch_bytes(P, src_max_h, src_pitch, cell, canvases) bytes, 16-byte aligned */
    int32_t* pages;                 /* out [P][ABC_SCAN_NPAGE] */
    int32_t* drawings;              /* out [canvases][ABC_SCAN_NDRAWING] */
    int32_t* total;                 /* out [2]: canvases written, kept groups of all pages */
    int32_t* labels_out;            /* optional out [P][cap_ch][cap_cw] (NULL: not written) */
    int32_t* canvas_out;            /* optional out [P][cap_ch][cap_cw] (NULL: not written) */
    int32_t canvases;               /* D, 1 .. 65535 */
    int32_t max_per_page;           /* K, 1 .. ABC_SCAN_SPLIT_MAX_PER_PAGE */
    int32_t cell;                   /* 8, 16, 32 or 64 */
    int32_t reach;                  /* 1 .. ABC_SCAN_SPLIT_MAX_REACH, in cells */
    int32_t min_ink;                /* >= 0 */
    int32_t keep_q8;                /* 0 .. 256 */
} abc_scan_split_desc;
int abc_split_scan_pages(const abc_scan_desc* d, const abc_scan_split_desc* q, abc_stream_t stream);
/* sizeof(abc_scan_split_desc), for a binding's mirror struct (as abc_scan_desc_size) */
int abc_scan_split_desc_size(void);
/* the bytes of abc_scan_split_desc.scratch for these capacities; ABC_EINVAL (negative) when one of them is outside the limits above */
int64_t abc_scan_split_scratch_bytes(int32_t P, int32_t src_max_h, int32_t src_pitch, int32_t cell, int32_t D);

/* Stroke width of a binary drawing, normalised (csrc/stroke.hip): peel it toward its skeleton, then grow it
 * back to a chosen width.  The augmentation the reference leaves commented out (utils.py:65-71: sm.thin, then sm.dilation with
 * sm.disk(1)) as a device stage; synthetic._line's lines of 3 pixels are a one-pixel skeleton dilated by disk(1).
 * src and dst are f32 [B][1][S][S] and may be the same buffer (otherwise they must not overlap).  A pixel is ink iff its value is
 * > 0.5f (a NaN is paper); the output is exactly 0.0f or 1.0f; pixels outside the canvas are paper.  Per image, in this order:
 *   despeckle  (drop_isolated 0 / 1) every ink pixel with no ink among its eight neighbours is deleted, all at once.
 *   thin       max_iter 0: none; k >= 1: at most k iterations; ABC_STROKE_UNTIL_STABLE: until stable.  One iteration is
 *              subiteration A, then subiteration B; each reads the state as it was before that subiteration and deletes all the
 *              pixels it flags at once.  Neighbours clockwise from north: p2 = N, p3 = NE, p4 = E, p5 = SE, p6 = S, p7 = SW,
 *              p8 = W, p9 = NW (north is the row above, west the column before).
 *                C  = (!p2 & (p3 | p4)) + (!p4 & (p5 | p6)) + (!p6 & (p7 | p8)) + (!p8 & (p9 | p2))
 *                N1 = (p9 | p2) + (p3 | p4) + (p5 | p6) + (p7 | p8),  N2 = (p2 | p3) + (p4 | p5) + (p6 | p7) + (p8 | p9)
 *                N  = min(N1, N2),  m_A = (p6 | p7 | !p9) & p8,  m_B = (p2 | p3 | !p5) & p4
 *              an ink pixel is deleted when C == 1, 2 <= N <= 3 and m == 0 (the Guo-Hall two-subiteration rule, the family of
 *              skimage.morphology.thin; bit-identity with skimage is NOT claimed: none was at hand to check against).
 *              Thinning stops after the first iteration that deletes nothing (that iteration is counted; converged = 1), and
 *              after max_iter iterations (converged = 1 only if the last one deleted nothing).  max_iter 0: 0 iterations,
 *              converged = 0.
 *   dilate     radius 0 .. 3: a pixel is ink iff some ink pixel lies at an offset (dy, dx) from it with dy^2 + dx^2 <= radius^2
 *              (the disk(r) footprints of 1, 5, 13 and 29 pixels), clipped at the canvas.
 *   stats      int32 [B][ABC_STROKE_NSTAT] (abc_stroke_stat order): iterations, converged, ink_in (after the > 0.5 cut), ink_out,
 *              skipped.
 *   skip       optional (NULL: none): image b is skipped when skip[b * skip_stride] != 0 (skip_stride in int32 words, >= 1): its
 *              pixels are carried from src to dst bit for bit -- in place, nothing is written: a NaN image stays NaN -- and its
 *              stats row reads 0, 0, 0, 0, 1.
 * One launch on the stream, one workgroup per image (the bit-packed image lives in LDS), no allocation, no sync, no parallel
 * branch (capturable).  ABC_EINVAL: a null or misaligned pointer (src, dst: 16 bytes), B < 1, radius outside 0 .. 3,
 * max_iter < -1, drop_isolated outside 0 / 1, S not a multiple of 8 in 8 .. ABC_STROKE_MAX_SIZE, src and dst overlapping
 * without being equal. */
enum { ABC_STROKE_UNTIL_STABLE = -1, ABC_STROKE_MAX_SIZE = 1024 };
enum abc_stroke_stat { ABC_STROKE_ITERATIONS = 0, ABC_STROKE_CONVERGED, ABC_STROKE_INK_IN, ABC_STROKE_INK_OUT, ABC_STROKE_SKIPPED,
                       ABC_STROKE_NSTAT };
typedef struct abc_stroke_desc {
    const float* src;               /* [B][1][S][S] f32, 16-byte aligned */
    float* dst;                     /* [B][1][S][S] f32, 16-byte aligned; may equal src */
    int32_t B, S;                   /* B >= 1; S a multiple of 8, 8 <= S <= ABC_STROKE_MAX_SIZE */
    int32_t drop_isolated;          /* 0 / 1 */
    int32_t max_iter;               /* 0, k >= 1 or ABC_STROKE_UNTIL_STABLE */
    int32_t radius;                 /* 0 .. 3 */
    int32_t skip_stride;            /* int32 words between the skip words of two images (>= 1 when skip is given) */
    const int32_t* skip;            /* optional device words, image b at skip[b * skip_stride]; non-zero: leave the image alone */
    int32_t* stats;                 /* out [B][ABC_STROKE_NSTAT] */
} abc_stroke_desc;
int abc_normalize_strokes(const abc_stroke_desc* d, abc_stream_t stream);
/* sizeof(abc_stroke_desc), for a binding's mirror struct (as abc_scan_desc_size) */
int abc_stroke_desc_size(void);

/* The capacities of the SMILES decoder's stages below, the sizes of their kernels' LDS arrays (a launch with more is ABC_EINVAL):
 * cap_atoms of extract, assemble and graph score; bond peaks per image abc_extract_peaks expands; max_atoms and max_bonds of the
 * graph score; cap_atoms and max_atoms of the graph similarity and of the graph identity. */
enum abc_decoder_limit { ABC_MAX_CAP_ATOMS = 2048, ABC_MAX_BOND_PEAKS = 4096, ABC_MAX_SCORE_RECORD = 1024, ABC_MAX_SIM_ATOMS = 512,
                         /* cap_atoms of abc_write_smiles: the per-atom LDS arrays of its walk, as many as the similarity's */
                         ABC_MAX_SMILES_ATOMS = ABC_MAX_SIM_ATOMS };

/* Candidate extraction for the SMILES decoder (img2smiles2.py:113-191; replaces its per-pixel .cpu().item() loops):
 * from the NMS masks of abc_nms_peaks and the raw head maps (all NCHW f32) to compact ordered lists per image.
 *   atoms[b][i] = (x, y, type, charge, hs)      raster order, greedy suppression within squared distance < 4
 *   bonds[b][i] = (x, y, omega bin, type), bond_rho[b][i] = |rho|   raster order of bond peaks, bins ascending,
 *                                                 a bin kept unless its opposite direction wins (lines 141-157)
 *   which bins are tried is omega_rule:
 *     ABC_OMEGA_RAW   (0, the default: img2smiles2.py:139) every bin whose RAW omega logit is non-zero -- the reference computes
 *                     the omega peak mask (img2smiles2.py:73-79) and does not read it;
 *     ABC_OMEGA_PEAKS (1: img2smiles.py:139, img2smiles3.py:140) every bin k with
 *                     v[k] == max(v[(k+59)%60], v[k], v[(k+1)%60]) && v[k] > -1   (the mask of img2smiles3.py:75-81);
 *                     a peak whose logit is exactly 0 is tried.  The kernel recomputes the mask from the raw logits with
 *                     abc_nms_peaks' comparison (on finite logits the kept bins are a subset of its omega_mask); omega_mask
 *                     itself is not an input.
 *   counts[b]   = (atom peaks, atoms accepted, bond peaks, bond candidates) -- true totals; the lists hold at most
 *                 cap_atoms / cap_bonds entries (and at most 4096 bond peaks per image are expanded).
 * x = row, y = column as in the reference. */
enum abc_omega_rule { ABC_OMEGA_RAW = 0, ABC_OMEGA_PEAKS = 1 };
typedef struct abc_extract_desc {
    const float* atom_mask; const float* bond_mask;               /* [B][1][h][w] */
    const float* types; const float* charges; const float* hs;    /* [B][14|3|2][h][w] logits */
    const float* btypes; const float* rho; const float* omega;    /* [B][360|60|60][h][w] raw maps */
    int32_t B, h, w, cap_atoms, cap_bonds;                        /* cap_atoms <= 2048 */
    int32_t* counts;      /* [B][4] */
    int32_t* atoms;       /* [B][cap_atoms][5] */
    int32_t* bonds;       /* [B][cap_bonds][4] */
    float* bond_rho;      /* [B][cap_bonds] */
    int32_t* work;        /* scratch, abc_extract_work_ints() int32 */
    uint64_t* work_masks; /* scratch, abc_extract_work_masks() uint64 */
    /* decode mode (InferenceRunner(decode=True)): the bond type of a (bin, pixel) from the heads kernel's arg-max map
     * (abc_conv_desc.head_aux_mode 3, uint8 [B][60][h][w]) instead of six raw planes -- btypes may then be NULL; rho may be the |rho|
     * map (the kernel takes the absolute value either way) */
    const uint8_t* btype_idx;
    int32_t omega_rule;   /* enum abc_omega_rule; any other value: ABC_EINVAL at call time.  A zeroed descriptor is ABC_OMEGA_RAW */
} abc_extract_desc;
int64_t abc_extract_work_ints(const abc_extract_desc* d);
int64_t abc_extract_work_masks(const abc_extract_desc* d);
int abc_extract_peaks(const abc_extract_desc* d, abc_stream_t stream);

/* Graph assembly for the SMILES decoder (img2smiles2.py:193-311): from the candidate lists of abc_extract_peaks (read in place)
 * to the molecule the reference hands to its mol-block writer.  One workgroup per image, float64 decisions in the reference's
 * operation order (csrc/assemble.hip), no allocation, no sync.
 *   bond ends    every candidate attaches to two accepted atoms (arg-min of the reference's two distances, first minimum wins);
 *   edge filter  a candidate with both ends on one atom (or rho == 0 / not finite) is dropped; of the rest the FIRST of every unordered atom pair stays;
 *   repair       an atom whose valence count exceeds its type's maximum becomes O, N, C, P, S, Cl for a count of 2..7;
 *   compaction   atoms no kept bond touches are dropped, the rest are numbered from 1 in list order;
 *   implicit H   atoms at a kept aromatic bond that are not carbon and have hs != 0, in order of first appearance.
 * mol_counts[b] = (atoms, bonds, implicit-H entries, status bits).  ABC_MOL_EMPTY: no atom peak or no bond peak (the
 * reference's results.append(None)); ABC_MOL_TRUNCATED: the extractor truncated a list or cap_mol_bonds was hit (the stored
 * molecule is then built from the truncated lists).  Bond peaks without a surviving candidate give zero atoms and zero bonds. */
enum abc_mol_status { ABC_MOL_EMPTY = 1, ABC_MOL_TRUNCATED = 2 };
/* the bits abc_write_molblocks and abc_write_smiles add to the two above in their own status words (never in mol_counts);
 * RING_LIMIT is the SMILES writer's alone */
enum abc_text_status { ABC_TEXT_BAD_ROW = 4, ABC_TEXT_OVERFLOW = 8, ABC_TEXT_RING_LIMIT = 16 };
typedef struct abc_assemble_desc {
    const int32_t* counts;    /* [B][4]            as abc_extract_desc.counts */
    const int32_t* atoms;     /* [B][cap_atoms][5] */
    const int32_t* bonds;     /* [B][cap_bonds][4] */
    const float* bond_rho;    /* [B][cap_bonds] */
    const double* trig;       /* device [2][60]: cos, then sin, of k * (pi / 30) + pi / 60 - pi / 2 (computed by the caller) */
    int32_t B, cap_atoms, cap_bonds, cap_mol_bonds;   /* cap_atoms 1..2048 */
    int32_t* mol_counts;      /* [B][4] */
    int32_t* mol_atoms;       /* [B][cap_atoms][5]      (x, y, vocabulary index after repair, charge VALUE, hs) */
    int32_t* mol_bonds;       /* [B][cap_mol_bonds][4]  (end 1, end 2 (1-based), order 1..6, index of the source candidate) */
    int32_t* mol_implh;       /* [B][cap_atoms]         1-based atom indices */
    int32_t* work;            /* scratch, abc_assemble_work_ints() int32 */
} abc_assemble_desc;
int64_t abc_assemble_work_ints(const abc_assemble_desc* d);
int abc_assemble_graphs(const abc_assemble_desc* d, abc_stream_t stream);

/* The 17 training meters of train.py:145-215 (each an AverageMeter.update(num/den, den), meter.py:12-16), from the
 * NCHW f32 head maps and the targets of the loss; replaces 34 host round trips per step by one device-side table.
 * Meter order: atom_targets {precision, precision3, recall, recall3}, atom_types_acc, atom_charges_acc, atom_hs_acc,
 * bond_targets {precision, precision3, recall, recall3}, bond_types_acc, bond_rhos_mae, bond_omega {precision,
 * recall3, recall, precision3}.  last[2i], last[2i+1] = (num, den) of this batch; totals += the same. */
typedef struct abc_metrics_desc {
    const float* logits[8];
    const float* t_atom; const float* t_types; const float* t_charges; const float* t_hs; const float* t_bond;
    const float* t_btypes; const double* t_rho; const double* t_omega;
    int32_t B, h, w;
    uint8_t* peaks;    /* scratch [2][B][h][w] */
    double* partial;   /* scratch [abc_metrics_blocks][24] */
    double* totals;    /* [17][2] running (sum, count), accumulated in place */
    double* last;      /* [17][2] */
} abc_metrics_desc;
int abc_metrics_blocks(const abc_metrics_desc* d);
int abc_metrics_update(const abc_metrics_desc* d, abc_stream_t stream);

/* The evaluation tables of test_accuracy.py:105-298 from what an inference step leaves on the device: the 3x3 centre masks,
 * the omega-bin mask and |rho| of abc_nms_peaks (the raw-logit "> -1" NMS, not the "> 0.25" of the training meters), the
 * logits of the atom heads, the bond-type head as raw planes or as its arg-max map, and the eight target maps.  One pass,
 * one thread per map pixel (csrc/eval_tables.hip): target planes are read everywhere, predictions only where a target
 * gives them weight.  No allocation, no sync: it may sit inside a captured graph.
 *   counts[301] (uint64, exact, independent of the order of the workgroups):
 *     [  0.. 41] atom_det[14][3]  (tp, fp, fn) of the atom centres by the pixel's target class (arg max of t_types,
 *                                 first index on ties, 0 where every plane is 0):
 *                                 tp = A & dil3(Ta), fp = A & !dil3(Ta), fn = Ta & !dil3(A)   (dil3: zero-padded 3x3 max)
 *     [ 42.. 59] bond_det[6][3]   the same for the bond centres, class = arg max over types of the sum over the bins
 *     [ 60..255] type[14][14]     confusion C[t][p] += #{target planes == 1} with t / p the arg max of targets / logits
 *     [256..264] charge[3][3]
 *     [265..300] btype[6][6]      per (pixel, omega bin), channel = type * 60 + bin
 *     The reference's (tp, tn, fp, fn) of class i are C[i][i], total - row i - column i + C[i][i], column i - C[i][i],
 *     row i - C[i][i].
 *   meters[17][2]: (num, den) of the 17 meters in the order of abc_metrics_desc, inference flavour (lines 188-269).
 * `last` holds this call alone, `totals` the running plain sums (a multi-rank caller may all-reduce them). */
enum { ABC_EVAL_NCOUNT = 301 };
typedef struct abc_eval_desc {
    const float* atom_mask; const float* bond_mask;              /* [B][1][h][w], 0 / 1 */
    const float* omega_mask; const float* rho_abs;               /* [B][60][h][w]: 0 / 1, |rho| */
    const float* types; const float* charges; const float* hs;   /* [B][14|3|2][h][w] logits */
    /* the bond-type prediction: exactly one of the raw planes [B][360][h][w] and the arg-max map uint8 [B][60][h][w] of
     * decode mode (abc_conv_desc.head_aux_mode 3) */
    const float* btypes; const uint8_t* btype_idx;
    const float* t_atom; const float* t_types; const float* t_charges; const float* t_hs; const float* t_bond;
    const float* t_btypes; const double* t_rho; const double* t_omega;
    const int32_t* n_valid;    /* optional DEVICE int32: only images 0 .. *n_valid - 1 count (clamped to 0 .. B); NULL: all B */
    int32_t B, h, w;
    double* partial;           /* scratch [abc_eval_tables_blocks][24] */
    uint64_t* counts_last; uint64_t* counts_totals;   /* [ABC_EVAL_NCOUNT] */
    double* meters_last; double* meters_totals;       /* [17][2] */
} abc_eval_desc;
int abc_eval_tables_blocks(const abc_eval_desc* d);
int abc_eval_tables_update(const abc_eval_desc* d, abc_stream_t stream);
/* as abc_eval_tables_update; target_flags = abc_raster_desc.group_flags of the rasteriser that drew d's target maps
 * (uint32 [B * h * w / 32]); h * w a multiple of 32.  In a group without bits 0-3 no atom-side target plane is read, in one
 * without bits 4-7 no bond-side plane: the maps must be zero there, as the rasteriser leaves them.  counts_* and meters_* are
 * the dense call's, bit for bit. */
int abc_eval_tables_update_sparse(const abc_eval_desc* d, const uint32_t* target_flags, abc_stream_t stream);
/* sizeof(abc_eval_desc), for a binding's mirror struct (this descriptor is not part of abc_sizeof's list) */
int abc_eval_desc_size(void);

/* The score AFTER assembly: how many assembled molecules (abc_assemble_graphs, read in place) are the annotated molecule
 * (raster.parse_graph records).  One workgroup per image, integer arithmetic only, no allocation, no sync (csrc/graph_score.hip).
 *   T        the annotated atoms that occur in at least one record bond (the assembler drops unbonded atoms too);
 *   P        the molecule's atoms;  near_P(a) / near_T(p): the atom of the other side at the least squared cell distance, the
 *            lowest row / record index on ties, defined only within radius^2;
 *   located  a in T and p in P that are each other's nearest;
 *   matched  a located pair with the same symbol (vocabulary index 0 reads as carbon on the predicted side; an annotated
 *            element of -1, outside the vocabulary, never matches) and the same charge value;
 *   paired   a molecule bond whose two ends are located and whose annotated pair the record lists (a record that lists a
 *            pair twice answers with its first listing);  matched: its order is also the record's code.
 * rows[b] (overwritten by every call; all zero for b >= *n_valid) and totals (+= the column sums, 64-bit integer atomics:
 * exact in any launch order) have the ABC_GS_* columns.  counted is 1 for every image below n_valid.  An ABC_MOL_EMPTY image
 * adds none = 1, atoms_true and bonds_true, and nothing else; a truncated molecule is scored as stored, with truncated = 1.
 * atoms_equal: atoms_matched == |T| == atoms_pred; bonds_equal: bonds_matched == bonds_true == bonds_pred; exact: both. */
enum { ABC_GS_COUNTED = 0, ABC_GS_NONE, ABC_GS_TRUNCATED, ABC_GS_EXACT, ABC_GS_ATOMS_EQUAL, ABC_GS_BONDS_EQUAL, ABC_GS_ATOMS_TRUE,
       ABC_GS_ATOMS_PRED, ABC_GS_ATOMS_LOCATED, ABC_GS_ATOMS_MATCHED, ABC_GS_BONDS_TRUE, ABC_GS_BONDS_PRED, ABC_GS_BONDS_PAIRED,
       ABC_GS_BONDS_MATCHED, ABC_GS_NCOL = 14 };
typedef struct abc_graph_score_desc {
    const int32_t* mol_counts;   /* [B][4]                 as abc_assemble_desc.mol_counts */
    const int32_t* mol_atoms;    /* [B][cap_atoms][5]      (x, y, vocabulary index, charge value, hs) */
    const int32_t* mol_bonds;    /* [B][cap_mol_bonds][4]  (end 1, end 2 (1-based), order, source candidate) */
    const int32_t* rec_atoms;    /* [B][max_atoms][4]      (x, y, vocabulary index or -1, charge value) */
    const int32_t* rec_bonds;    /* [B][max_bonds][3]      (i, j (0-based, i < j), code 1..6) */
    const int32_t* rec_counts;   /* [2][B]                 atoms, then bonds, of every record */
    const int32_t* n_valid;      /* optional DEVICE int32: only images 0 .. *n_valid - 1 count (clamped to 0 .. B); NULL: all B */
    int32_t B, cap_atoms, cap_mol_bonds, max_atoms, max_bonds;   /* cap_atoms 1..2048, max_atoms 1..1024, max_bonds 1..1024 */
    int32_t radius;              /* >= 0, in cells */
    int32_t* rows;               /* [B][ABC_GS_NCOL] */
    uint64_t* totals;            /* [ABC_GS_NCOL] */
} abc_graph_score_desc;
int abc_graph_score_update(const abc_graph_score_desc* d, abc_stream_t stream);
/* sizeof(abc_graph_score_desc), for a binding's mirror struct (as abc_eval_desc_size: not part of abc_sizeof's list) */
int abc_graph_score_desc_size(void);

/* The GRADED score after assembly, free of positions: the similarity of the atom environments of the assembled molecule and of
 * the annotated one (the stand-in for the Dice similarity of radius-3 Morgan fingerprints of cal_acc.py:38-43; DESIGN.md section 7
 * lists what of RDKit's fingerprint it leaves out).  One workgroup per image, uint64 wrapping arithmetic only, no allocation, no
 * sync (csrc/graph_sim.hip).  The molecule rows and the records are abc_graph_score_desc's, read the same way.
 *   atoms    molecule: all mol_counts[b][0] rows; record: the set T of abc_graph_score_update (atoms some valid bond row names);
 *   class    of a vocabulary index t: 1 for t = 0 (carbon), t for 1..13, 0 ("unknown", equal only to itself) for anything else
 *            (a record's -1); the charge value counts as stored, hs does not (a record has none);
 *   bonds    a row is valid when both ends are in range and differ; order class: codes 5 and 6 are 1 (a wedge is a single bond),
 *            1..4 stay, anything else is 0; a pair listed twice counts twice (a multigraph); no degree cap;
 *   mix(x)   the splitmix64 finaliser: x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31;
 *   id_0[a]  mix(mix(mix(class + 1) + (uint64)(int64)charge) + degree), degree = the valid rows naming a;
 *   id_r[a]  mix(mix(id_{r-1}[a] + r) + acc), acc = the sum over the valid rows (a, j, order class o) of mix(mix(id_{r-1}[j]) + o)
 *            (the neighbour term is mixed twice: with one mix it is the self term's function at r = o = 1).
 * The fingerprint of a side is the multiset {id_r[a] : r = 0..3}, 4 n elements.  envs_common is the size of the multiset
 * intersection, dice_q20 = floor(2 envs_common 2^20 / (envs_pred + envs_true)) (0 for an empty denominator), dice_one: common ==
 * pred == true > 0.  size_equal: the atom counts and the valid bond counts are equal; refine_equal: size_equal, and the multisets
 * of id_T are equal after T = min(n, 64) rounds of the same recurrence -- colour refinement, necessary for isomorphism and not
 * sufficient (decalin and bicyclopentyl pass): an UPPER bound of "the same molecule", as ABC_GS_EXACT is the positional lower one.
 * rows[b] (overwritten by every call; all zero for b >= *n_valid) and totals (+= the column sums, 64-bit integer atomics) have
 * the ABC_SIM_* columns.  An ABC_MOL_EMPTY image adds counted, none and envs_true, and nothing else.  The mean similarity is
 * totals[dice_q20] / 2^20 / totals[counted]. */
enum { ABC_SIM_COUNTED = 0, ABC_SIM_NONE, ABC_SIM_TRUNCATED, ABC_SIM_SIZE_EQUAL, ABC_SIM_REFINE_EQUAL, ABC_SIM_DICE_ONE,
       ABC_SIM_ATOMS_PRED, ABC_SIM_ATOMS_TRUE, ABC_SIM_ENVS_PRED, ABC_SIM_ENVS_TRUE, ABC_SIM_ENVS_COMMON, ABC_SIM_DICE_Q20,
       ABC_SIM_NCOL = 12, ABC_SIM_IDS = 2048 };
typedef struct abc_graph_similarity_desc {
    const int32_t* mol_counts;   /* [B][4]                 as abc_graph_score_desc */
    const int32_t* mol_atoms;    /* [B][cap_atoms][5] */
    const int32_t* mol_bonds;    /* [B][cap_mol_bonds][4] */
    const int32_t* rec_atoms;    /* [B][max_atoms][4] */
    const int32_t* rec_bonds;    /* [B][max_bonds][3] */
    const int32_t* rec_counts;   /* [2][B] */
    const int32_t* n_valid;      /* optional DEVICE int32, as abc_graph_score_desc */
    int32_t B, cap_atoms, cap_mol_bonds, max_atoms, max_bonds;   /* cap_atoms 1..512, max_atoms 1..512; the bond capacities >= 1 */
    int32_t* rows;               /* [B][ABC_SIM_NCOL] */
    uint64_t* totals;            /* [ABC_SIM_NCOL] */
    /* optional (debug): [B][2][ABC_SIM_IDS], the fingerprint ids of the molecule, then of the record, of every image below
     * *n_valid: id_r of the side's a-th atom (the record's: the a-th of T in index order) at r * n + a, zero past 4 n */
    uint64_t* ids_out;
} abc_graph_similarity_desc;
int abc_graph_similarity_update(const abc_graph_similarity_desc* d, abc_stream_t stream);
/* sizeof(abc_graph_similarity_desc), for a binding's mirror struct (as abc_graph_score_desc_size) */
int abc_graph_similarity_desc_size(void);

/* The CERTAIN score after assembly, free of positions: is the assembled molecule the annotated one?  An individualise-and-refine
 * isomorphism test per image between ABC_GS_EXACT (the positional lower bound) and ABC_SIM_REFINE_EQUAL (the upper one).  One
 * workgroup per image, uint64 wrapping arithmetic only, no allocation, no sync (csrc/graph_ident.hip; its executable form is
 * tests/graphident_oracle.py).  The graphs -- atoms, classes, charges, valid rows, order classes, multigraph -- mix, id_0 and the
 * round id_r are abc_graph_similarity_update's, word for word; the rows and records are read the same way.
 *   sizes     the atom counts and the valid-bond counts are equal (size_equal), else `different`;
 *   indiv     indiv(id, level) = mix(mix(id) + 0x9E3779B97F4A7C15 (level + 1)), the id of the atom individualised at `level`;
 *   molecule  walks ONE path to a discrete colouring.  Per level: rounds (r counts on through the levels) until one no longer
 *             raises the number of distinct ids -- that round is counted, a level has at most n; the level's round count, the sum
 *             of mix(id) over the atoms and the class count are recorded; not discrete: the cell is the non-singleton class with
 *             the least id VALUE, its lowest-index atom v gets id[v] = indiv(id[v], level), and the next level starts (its class
 *             count before the first round is taken as the recorded one plus 1);
 *   record    is searched depth first doing what the molecule recorded: per level the same number of rounds, after which class
 *             count and sum must equal the record's (a mismatch proves the branch wrong, the ids being functions of structure
 *             alone); the candidates of a level are the record atoms whose id is the recorded cell id, in index order, each
 *             individualised as above (a try); a failed or exhausted level is a backtrack: one level up, the ids rebuilt by
 *             replaying the choices from id_0;
 *   leaf      both colourings discrete: atoms are mapped by equal id, then VERIFIED -- class and charge of every atom, and the
 *             multiset of (mapped end, mapped end, order class) of the molecule's valid rows against the record's, by counting.
 *             Verified: `same`, certain whatever the hashes did.  Not verified: the search goes on.  Exhausted: `different`;
 *   budgets   max_rounds is checked before every round of either side (replays included), max_tries before every try; running out
 *             is `undecided`.  0 selects the defaults below; every loop is bounded by n, a budget or a capacity.
 *             The defaults were chosen with the oracle.  The largest seen on any test fixture: tries = 254 and rounds = 1018 (170
 *             disjoint C-C-C, 510 atoms; a 512-carbon chain takes 1008 rounds, a 512-carbon ring 988).  Every pair of the trained
 *             fixture under both omega rules stays at 2 levels, 0 tries and 7 rounds (profiles/r15_identity.md).
 * rows[b] (overwritten by every call; all zero for b >= *n_valid) and totals (+= the column sums, 64-bit integer atomics) have the
 * ABC_IDENT_* columns: levels = the molecule's individualisations, tries, backtracks, rounds (both sides) = the work of the image.
 * An ABC_MOL_EMPTY image adds counted and none, and nothing else; of every other counted image exactly one of same, different and
 * undecided is 1 (a size mismatch is `different` with zero work).  Two sides without atoms are `same`.
 * map_out (optional) is the WITNESS: for a `same` image, the ORIGINAL record atom index of every molecule atom; -1 in every other
 * word of the [B][cap_atoms] table, which every launch writes entirely. */
enum { ABC_IDENT_DEFAULT_TRIES = 4096, ABC_IDENT_DEFAULT_ROUNDS = 16384 };
enum { ABC_IDENT_COUNTED = 0, ABC_IDENT_NONE, ABC_IDENT_TRUNCATED, ABC_IDENT_SIZE_EQUAL, ABC_IDENT_SAME, ABC_IDENT_DIFFERENT,
       ABC_IDENT_UNDECIDED, ABC_IDENT_LEVELS, ABC_IDENT_TRIES, ABC_IDENT_BACKTRACKS, ABC_IDENT_ROUNDS,
       ABC_IDENT_NCOL = 11 };
typedef struct abc_graph_identity_desc {
    const int32_t* mol_counts;   /* [B][4]                 as abc_graph_score_desc */
    const int32_t* mol_atoms;    /* [B][cap_atoms][5] */
    const int32_t* mol_bonds;    /* [B][cap_mol_bonds][4] */
    const int32_t* rec_atoms;    /* [B][max_atoms][4] */
    const int32_t* rec_bonds;    /* [B][max_bonds][3] */
    const int32_t* rec_counts;   /* [2][B] */
    const int32_t* n_valid;      /* optional DEVICE int32, as abc_graph_score_desc */
    int32_t B, cap_atoms, cap_mol_bonds, max_atoms, max_bonds;   /* cap_atoms 1..512, max_atoms 1..512; the bond capacities >= 1 */
    int32_t max_tries, max_rounds;   /* >= 1, or 0: ABC_IDENT_DEFAULT_TRIES / ABC_IDENT_DEFAULT_ROUNDS; negative: ABC_EINVAL */
    int32_t* rows;               /* [B][ABC_IDENT_NCOL] */
    uint64_t* totals;            /* [ABC_IDENT_NCOL] */
    int32_t* map_out;            /* optional: [B][cap_atoms], the witness */
} abc_graph_identity_desc;
int abc_graph_identity_update(const abc_graph_identity_desc* d, abc_stream_t stream);
/* sizeof(abc_graph_identity_desc), for a binding's mirror struct (as abc_graph_similarity_desc_size) */
int abc_graph_identity_desc_size(void);

/* A CANONICAL ATOM ORDER per image: the order of the least leaf of an individualise-and-refine search that visits every branch
 * (csrc/graph_canon.hip; its host form is decode.canonical_labelling, its test oracle tests/graphcanon_oracle.py; DESIGN.md section
 * 7).  With it the text rules of abc_write_smiles and abc_write_molblocks, pure functions of atom order, graph and implicit-H list,
 * write equal strings if and only if the graphs are equal.  NOT RDKit's canonical order.  One workgroup of 256 threads per image,
 * uint64 wrapping arithmetic only, no global atomics, no allocation, no sync; every branch depends on values all threads hold alike,
 * every index read from a row is range-checked, every loop is bounded by n, a budget or a capacity.
 *   graph     ONE side of abc_graph_identity_update's graphs, built the same way (atom classes, order classes with wedges folded
 *             to 1, a pair listed twice counts twice, mix, id_0, the round, indiv): the molecule rows when mol_counts is given
 *             (every atom; EMPTY and TRUNCATED are copied into the status), else the graph records (only the atoms some valid bond
 *             row names, in index order).  Giving both sides, or neither, is ABC_EINVAL;
 *   tag       1 for a molecule atom that mol_implh lists (an entry in 1..n among the first mol_counts[2], clamped to cap_atoms), 0
 *             otherwise, for records and when mol_implh is NULL.  id_0 = mix(id_0 + 0xD6E8FEB86659FD93 * tag) for tag != 0; with all
 *             tags 0 the ids are the identity's, bit for bit;
 *   tree      a node is a sequence of individualised atoms v_1 .. v_k; its colouring starts at id_0; for level 0 .. k: rounds (r
 *             counts on through the levels) until one no longer raises the class count -- that round is counted, a level has at most
 *             n -- then the level's TRACE (rounds, classes, wrapping sum of mix(id)), then id[v_(l+1)] = indiv(id, l).  The target
 *             cell of a colouring that is not discrete is the non-singleton class of the least id VALUE; the children are its atoms
 *             in index order; a leaf is a discrete colouring;
 *   leaf      rank(a) = the number of atoms with a smaller id;
 *             h = sum over the atoms of mix(mix(mix(mix(rank + 1) + class + 1) + charge) + tag)
 *               + sum over the valid rows of mix(mix((lower rank << 32 | higher rank) + 0xC2B2AE3D27D4EB4F) + order class), wrapping;
 *             trace and h are functions of the relabelled graph alone.  The canonical leaf is the LEAST under lexicographic
 *             comparison of (trace_0, trace_1, .., h), a trace compared as its tuple, numbers ascending; the order is its ranks;
 *   search    depth first, backtracking by replaying the choices from id_0, with two prunings that cannot change the result:
 *             TRACE -- while the path has equalled the best leaf's traces, a level whose trace is greater drops the branch, one that
 *             is less makes the path strictly better (no further comparison; its leaf replaces the best).  AUTOMORPHISM -- a leaf
 *             whose whole key equals the best's is mapped onto it by equal id (through the LDS table) and the map VERIFIED as the
 *             identity's leaf is: class, charge and tag of every atom, the multiset of (mapped end, mapped end, order class) by
 *             counting.  Verified: gamma is an automorphism, certain whatever the hashes did; it fixes the stack's prefix through
 *             the level p where the path left the best's; for every level l <= min(p, ABC_CANON_ORBIT_LEVELS) x ~ gamma(x) is merged
 *             into that level's orbit table (a union-find over atoms in LDS, reset when the level is entered anew), and the search
 *             returns at once to level p (the subtree left is the image of one already searched).  A child w of a node at a level
 *             <= ABC_CANON_ORBIT_LEVELS is skipped when a lower-indexed atom of its cell is in w's orbit there; deeper levels prune
 *             by trace only.  Not verified: two 64-bit sums collided -- the search stops with ABC_CANON_COLLISION;
 *   budgets   max_rounds is checked before every round (replays included), max_tries before every individualisation; 0 selects the
 *             defaults.  Running out sets ABC_CANON_UNDECIDED: the order is then that of the best leaf reached so far, a valid
 *             permutation, or the identity order if no leaf was reached.  Chosen with the oracle at capacity: a 512-carbon ring takes
 *             5 to 9 tries and 1483 to 2471 rounds (by numbering), a 512-carbon chain 2 tries and 1008 rounds; 170 disjoint C-C-C
 *             and 64 disjoint benzenes need a descent per sibling below the orbit levels and END UNDECIDED at these defaults;
 *   limits    cap_atoms (molecule side) or max_atoms (records) 1..512, else ABC_EUNSUPPORTED with nothing launched; bond rows stay
 *             out of LDS; cap_mol_bonds <= 4096 when the canonical rows are requested (ABC_EUNSUPPORTED);
 *   outputs   every word is written by every launch (cap = cap_atoms | max_atoms, cap_bonds = cap_mol_bonds | max_bonds):
 *             order [B][cap]: order[b][k] = the 0-based row (for a record: the original record index) of the atom at canonical
 *               position k, -1 beyond n;
 *             stats [B][ABC_CANON_NCOL]: the status bits, then the counters leaves, tries, rounds, levels_max, pruned_trace,
 *               pruned_orbit, automorphisms, improved (leaves that replaced a best one); an EMPTY image has only its status word;
 *             key [B][2]: h of the chosen order, then mix(mix(mix(n) + m) + sum over the chosen leaf's levels l of
 *               mix(mix(mix(mix(l + 1) + rounds_l) + classes_l) + sum_l)) -- a HASH: equal keys are necessary for equal graphs, not
 *               sufficient;
 *             cert_out (optional) [B][2 + cap + 3 cap_bonds]: n, m, the n atom words (charge << 5 | tag << 4 | class, wrapping: exact
 *               for |charge| < 2^26) in rank order, the m triples (lower rank, higher rank, order class) ascending, then -1.  This is
 *               the relabelled graph itself: equal cert_out IS equal graphs (0, 0, then -1 for an EMPTY image);
 *             out_counts, out_atoms, out_bonds, out_implh (molecule side, optional, all four or none; they must not overlap the
 *               inputs: ABC_EINVAL): the CANONICAL ROWS in the layouts of abc_assemble_desc -- mol_counts copied;
 *               out_atoms[k] = mol_atoms[order[k]]; in the bond rows both ends are renumbered (1-based) in place, end 1 stays end 1 so
 *               a wedge keeps its owner, order and source unchanged; the valid rows first, ascending by (lower end, higher end,
 *               original row), the rows the graph skipped after them verbatim; mol_implh renumbered, the entries in 1..n ascending,
 *               the others after them verbatim; zero past the (clamped) counts and for an EMPTY image.  */
enum { ABC_CANON_DEFAULT_TRIES = 4096, ABC_CANON_DEFAULT_ROUNDS = 16384, ABC_CANON_ORBIT_LEVELS = 8 };
enum abc_canon_status { ABC_CANON_EMPTY = 1, ABC_CANON_TRUNCATED = 2, ABC_CANON_UNDECIDED = 4, ABC_CANON_COLLISION = 8 };
enum { ABC_CANON_STATUS = 0, ABC_CANON_LEAVES, ABC_CANON_TRIES, ABC_CANON_ROUNDS, ABC_CANON_LEVELS_MAX, ABC_CANON_PRUNED_TRACE,
       ABC_CANON_PRUNED_ORBIT, ABC_CANON_AUTOMORPHISMS, ABC_CANON_IMPROVED, ABC_CANON_NCOL = 9 };
typedef struct abc_canon_desc {
    const int32_t* mol_counts;   /* [B][4]                 the molecule side (as abc_assemble_desc), or NULL */
    const int32_t* mol_atoms;    /* [B][cap_atoms][5] */
    const int32_t* mol_bonds;    /* [B][cap_mol_bonds][4] */
    const int32_t* mol_implh;    /* optional: [B][cap_atoms], the tags */
    const int32_t* rec_atoms;    /* [B][max_atoms][4]      the records side (as abc_graph_score_desc), or NULL */
    const int32_t* rec_bonds;    /* [B][max_bonds][3] */
    const int32_t* rec_counts;   /* [2][B] */
    int32_t B, cap_atoms, cap_mol_bonds, max_atoms, max_bonds;   /* the capacities of the side that is given */
    int32_t max_tries, max_rounds;   /* >= 1, or 0: ABC_CANON_DEFAULT_TRIES / ABC_CANON_DEFAULT_ROUNDS; negative: ABC_EINVAL */
    int32_t* order;              /* [B][cap] */
    int32_t* stats;              /* [B][ABC_CANON_NCOL] */
    int64_t* key;                /* [B][2] */
    int32_t* cert_out;           /* optional: [B][2 + cap + 3 cap_bonds] */
    int32_t* out_counts;         /* optional, molecule side: the canonical rows, [B][4] */
    int32_t* out_atoms;          /* [B][cap_atoms][5] */
    int32_t* out_bonds;          /* [B][cap_mol_bonds][4] */
    int32_t* out_implh;          /* [B][cap_atoms] */
} abc_canon_desc;
int abc_canonical_order(const abc_canon_desc* d, abc_stream_t stream);
/* sizeof(abc_canon_desc), for a binding's mirror struct (as abc_graph_identity_desc_size) */
int abc_canon_desc_size(void);

/* The STEREO ELEMENTS of every assembled molecule, perceived as a stage of its own (csrc/stereo.hip; the host form is
 * decode.stereo_elements): what the tetrahedral rule of abc_write_smiles_stereo and the double-bond rule of
 * abc_write_smiles_ez decide, by the same code -- qualification, the int64 determinant and cross products, the position range
 * 0..199999, the twin test and RING = not a bridge are stated once, in csrc/stereo_rules.hpp, for the writer and for this stage, which
 * also validates rows (the duplicate-pair test too) and counts hydrogens as the writer does -- written as a table that
 * abc_canonical_order_stereo reads.  One workgroup of 256 threads per image, the molecule side only, integers only,
 * no global atomics, no allocation, no sync; the rows are read in place and every index read from a row is range-checked.
 *   elements  [B][cap_atoms][ABC_STEREO_W], every word written by every launch; per atom row:
 *               [0]      the centre code as abc_smiles_stereo_desc.stereo_out defines it: 0, +1 / -1, 2 flat, 3 unqualified;
 *               [1..4]   for a +1 / -1 centre its neighbours' 0-based rows ascending, the hydrogen of a three-neighbour centre as -1
 *                        in the last place; -1 otherwise;
 *               [5]      for the atom that is the lower-index end of a candidate double bond, that bond row's code as
 *                        abc_smiles_ez_desc.ez_out defines it (+1 / -1, 2, 3, 4); 0 otherwise;
 *               [6..11]  for a +1 / -1 bond: the bond row, the partner, this end's one or two substituents ascending (-1 for none),
 *                        the partner's likewise; -1 otherwise;
 *             the NONE row (0, -1 x 4, 0, -1 x 6) past the atom count and for an image that is EMPTY or refused;
 *   stats     [B][4]: marked centres, marked double bonds, flat (both kinds), status -- the EMPTY / TRUNCATED bits of mol_counts and
 *             ABC_TEXT_BAD_ROW for rows abc_write_smiles refuses (the writer's ring limit is a limit of its text, not of the rows: it
 *             is not read here);
 *   limits    cap_atoms 1..ABC_MAX_SMILES_ATOMS, cap_mol_bonds 1..4096, else ABC_EUNSUPPORTED with nothing launched; a null buffer
 *             (mol_implh too) is ABC_EINVAL.
 * Not covered: what the two rules list as not covered; the records side (records carry no implicit-H list, so the hydrogen count,
 * and with it qualification, is not defined there). */
enum { ABC_STEREO_W = 12 };
typedef struct abc_stereo_desc {
    const int32_t* mol_counts;   /* [B][4] */
    const int32_t* mol_atoms;    /* [B][cap_atoms][5] */
    const int32_t* mol_bonds;    /* [B][cap_mol_bonds][4] */
    const int32_t* mol_implh;    /* [B][cap_atoms] */
    int32_t B, cap_atoms, cap_mol_bonds;
    int32_t* elements;           /* [B][cap_atoms][ABC_STEREO_W] */
    int32_t* stats;              /* [B][4] */
} abc_stereo_desc;
int abc_perceive_stereo(const abc_stereo_desc* d, abc_stream_t stream);
/* sizeof(abc_stereo_desc), for a binding's mirror struct */
int abc_stereo_desc_size(void);

/* The canonical ISOMERIC order: abc_canonical_order with the stereo elements as a third key (a second instantiation of the same
 * kernel; abc_canonical_order keeps its instructions).  Everything of abc_canon_desc holds -- tree, traces, trace pruning, budgets,
 * replay, h, key, cert_out, the stats columns, the canonical rows -- and:
 *   word      at a leaf, one byte per canonical position, centre part | double-bond part << 2, each 0 none, 1 for +1, 2 for -1.
 *             Centre part, for the atom a at the position: s(a) (elements[a][0]) times the sign of the permutation that sorts its up
 *             to four neighbours by rank, the hydrogen staying last.  Double-bond part, at the lower-RANK end of a marked double bond:
 *             its code times f(a) f(b), f(e) = -1 iff end e has two substituents and the lower-ranked one is not the lower-indexed
 *             one (the two lie on opposite sides: this is "lowest-rank substituents together / opposite").  An element whose indices
 *             are not atoms of the image is read as none;
 *   order     leaves are ordered by (traces, h, word), the word compared EXACTLY, position by position;
 *   equal h   the map onto the best leaf is verified as ever (failure: ABC_CANON_COLLISION).  Words equal: the map is an
 *             automorphism of the STEREO graph, merged into the orbit tables, and the search returns to the level where the paths
 *             parted.  Word smaller: the leaf becomes the best (counted in `improved`), nothing is merged, no jump.  Greater: a normal
 *             backtrack.  Orbit pruning so uses only automorphisms that keep the stereo; `automorphisms` counts those;
 *   rows      the canonical rows are written as ever (positions move with their atoms, end 1 stays end 1): s and the double-bond codes
 *             of abc_write_smiles_ez (tetrahedral != 0) on them ARE the word of the chosen leaf, so its text is equal if and only if
 *             the stereo graphs are equal (unless UNDECIDED or COLLISION).  All leaves of equal h relabel to one graph: cert_out, key
 *             and the plain text equal those of abc_canonical_order;
 *   stereo_search [B][4]: leaves with equal h and unequal word, stereo improvements, stereo automorphisms, 0.
 * The molecule side only: records with `elements` are ABC_EINVAL, as are a null elements or stereo_search. */
typedef struct abc_canon_stereo_desc {
    const int32_t* mol_counts;   /* the fields of abc_canon_desc, in its order */
    const int32_t* mol_atoms;
    const int32_t* mol_bonds;
    const int32_t* mol_implh;
    const int32_t* rec_atoms;    /* the records side: refused */
    const int32_t* rec_bonds;
    const int32_t* rec_counts;
    int32_t B, cap_atoms, cap_mol_bonds, max_atoms, max_bonds;
    int32_t max_tries, max_rounds;
    int32_t* order;
    int32_t* stats;
    int64_t* key;
    int32_t* cert_out;
    int32_t* out_counts;
    int32_t* out_atoms;
    int32_t* out_bonds;
    int32_t* out_implh;
    const int32_t* elements;     /* [B][cap_atoms][ABC_STEREO_W]: abc_perceive_stereo's table of the same rows */
    int32_t* stereo_search;      /* [B][4] */
} abc_canon_stereo_desc;
int abc_canonical_order_stereo(const abc_canon_stereo_desc* d, abc_stream_t stream);
/* sizeof(abc_canon_stereo_desc), for a binding's mirror struct */
int abc_canon_stereo_desc_size(void);

/* Aromaticity perception: the rows of one side copied with the bonds of every aromatic cycle set to order 4, so that a ring drawn with
 * alternating orders 1 / 2 and the same ring drawn with order 4 are one graph for abc_canonical_order, abc_write_smiles and the three
 * graph scores, which take the output in place of the input (csrc/aromatic.hip; host form decode.perceive_aromatic; DESIGN.md section
 * 7).  The rule is this project's own, a function of the graph alone, integers only; RDKit is not consulted and differs on azulene,
 * on 10-electron and larger systems and on a degree-2 `n` of an order-4 ring that carries a hydrogen.  One launch on the stream, one
 * workgroup of 256 threads per image, no atomics on global memory, no allocation, no sync, graph-capturable.
 *   graph     one side per call, as abc_canon_desc: the atoms of the side; the valid bond rows (molecule: both ends in 1..n and
 *             distinct; record: both in 0..n-1 and distinct); the order class of a code: 1, 2, 3, 4 themselves, 5 and 6 (wedges) class
 *             1, anything else class 0; degree = the number of valid rows at an atom; symbols by vocabulary index (0 and 1 are both
 *             carbon), an index outside 0..13 (a record's -1) is no symbol;
 *   candidate an atom whose symbol is one of B C N O P S Se, whose charge is in -1..1, whose degree is 2 or 3, none of whose rows has
 *             class 0 or 3, at most one of whose rows has class 2, and no two of whose rows name the same neighbour;
 *   cycle     a candidate cycle is a simple cycle of 5, 6 or 7 candidates along valid rows -- every one, the envelopes of fused rings
 *             included (degree <= 3 bounds the walk: there is no budget); a ring bond is a valid row on at least one of them;
 *   e(a)      the electrons of a candidate, from the INPUT classes, one value per atom; the first case that applies:
 *             (1) a has a class-2 row: 1 if that row is a ring bond; else 0 if its other end is one of N O S Se; else NONE;
 *             (2) with has4 = a has a class-4 row --  C: charge 0: 1 if has4 else NONE; -1: 2; +1: 0.   B: charge 0: 0; else NONE.
 *                 N, P: charge -1: 2; +1: 1 if has4 else NONE; 0 with has4: 2 at degree 3, 1 at degree 2; 0 without has4: 2.
 *                 O, S, Se: charge 0: 2; else NONE;
 *   aromatic  a candidate cycle without NONE whose e sum to exactly 6;
 *   output    every row on an aromatic cycle with order 4 (a wedge code 5 / 6 there becomes 4), every other row verbatim, invalid
 *             rows and class-0 rows included; atoms, counts and status bits copied.  One pass: nothing reads an order this pass wrote,
 *             so the result does not depend on numbering, row order or thread order;
 *   hydrogen  (molecule side) with h the hydrogen count of abc_write_smiles' text rule: an atom mol_implh does not list whose h is 1
 *             on the input rows and 0 on the output rows is appended to the list -- out_implh is the input's entries in their order,
 *             then the new ones ascending, out_counts[2] their number (new entries past cap_atoms, which only a list naming an atom
 *             twice can cause, are dropped); this keeps pyrrole [nH]1cccc1.  Records have no list: their side writes bonds only;
 *   limits    cap_atoms (molecule side) or max_atoms (records) 1..512, else ABC_EUNSUPPORTED with nothing launched; bond rows stay
 *             out of LDS: their capacity is free.  No output may overlap an input or another output (ABC_EINVAL);
 *   outputs   every word is written by every launch, zero past the (clamped) counts and for an EMPTY image:
 *             stats [B][ABC_AROM_NCOL]: the status bits (ABC_MOL_EMPTY, ABC_MOL_TRUNCATED, copied; 0 for a record), candidates,
 *               candidate cycles, aromatic cycles (each cycle once), rows whose order changed, atoms appended to the list;
 *             code_out (optional) [B][cap]: per atom ABC_AROM_NOT_CANDIDATE, ABC_AROM_NONE or e (NOT_CANDIDATE past n). */
enum { ABC_AROM_STATUS = 0, ABC_AROM_CANDIDATES, ABC_AROM_CYCLES, ABC_AROM_AROMATIC, ABC_AROM_ROWS_CHANGED, ABC_AROM_LISTED, ABC_AROM_NCOL = 6 };
enum { ABC_AROM_NOT_CANDIDATE = -2, ABC_AROM_NONE = -1 };
typedef struct abc_aromatic_desc {
    const int32_t* mol_counts;   /* [B][4]                 the molecule side (as abc_assemble_desc), or NULL */
    const int32_t* mol_atoms;    /* [B][cap_atoms][5] */
    const int32_t* mol_bonds;    /* [B][cap_mol_bonds][4] */
    const int32_t* mol_implh;    /* optional: [B][cap_atoms]; without it no atom counts as listed */
    const int32_t* rec_atoms;    /* [B][max_atoms][4]      the records side (as abc_graph_score_desc), or NULL */
    const int32_t* rec_bonds;    /* [B][max_bonds][3] */
    const int32_t* rec_counts;   /* [2][B] */
    int32_t B, cap_atoms, cap_mol_bonds, max_atoms, max_bonds;   /* the capacities of the side that is given */
    int32_t pad_;
    int32_t* stats;              /* [B][ABC_AROM_NCOL] */
    int32_t* code_out;           /* optional: [B][cap] */
    int32_t* out_counts;         /* molecule side, all four: the perceived rows, [B][4] */
    int32_t* out_atoms;          /* [B][cap_atoms][5] */
    int32_t* out_bonds;          /* [B][cap_mol_bonds][4] */
    int32_t* out_implh;          /* [B][cap_atoms] */
    int32_t* out_rec_bonds;      /* records side: [B][max_bonds][3] */
} abc_aromatic_desc;
int abc_perceive_aromatic(const abc_aromatic_desc* d, abc_stream_t stream);
/* sizeof(abc_aromatic_desc), for a binding's mirror struct (as abc_canon_desc_size) */
int abc_aromatic_desc_size(void);

/* The mol block text of the assembled molecules (generate_smiles.py:18-105), written on the device from the rows of
 * abc_assemble_graphs, read in place: the bytes that go into Chem.MolFromMolBlock, one copy per batch (csrc/molblock.hip; the
 * contract in full: DESIGN.md section 7).  Two launches on the stream, integers only, no atomics on global memory, no allocation,
 * no sync; deterministic in any launch order.
 *   text     the blocks of the batch back to back in image order, no terminator between them; image b is
 *            text[offsets[b] .. offsets[b+1]), byte for byte what decode.Molecule.from_device_rows(rows of b).molblock() gives
 *            (ASCII): every %3d / %4d is a MINIMUM width, a coordinate is px / 60 - 1 to four decimals computed as
 *            q = (2 |px - 60| 500 + 3) / 6 in integer division and printed q / 10000 "." (q % 10000, four digits), negative exactly
 *            when px < 60 (then after three blanks, else after four); bond ends, orders, charges and implicit-H entries are printed
 *            as stored (any int32); every count is clamped to its capacity first;
 *   index    offsets[0 .. B], then status[0 .. B-1];
 *   status   ABC_MOL_EMPTY / ABC_MOL_TRUNCATED copied from mol_counts (EMPTY: length 0; TRUNCATED: the text of the stored rows);
 *            ABC_TEXT_BAD_ROW: an atom row with a vocabulary index outside 0..13 or a position outside 0..199999, length 0;
 *            ABC_TEXT_OVERFLOW: an image is written only if the UNCLIPPED running total of the lengths through it is <= cap_text --
 *            the first image that does not fit and every image after it have length 0 and this bit, so what is written is a
 *            prefix of the batch;
 *   work     scratch int32 [B] (the length of every image, -1 for a refused row). */
typedef struct abc_molblock_desc {
    const int32_t* mol_counts;   /* [B][4]                 as abc_assemble_desc.mol_counts */
    const int32_t* mol_atoms;    /* [B][cap_atoms][5] */
    const int32_t* mol_bonds;    /* [B][cap_mol_bonds][4] */
    const int32_t* mol_implh;    /* [B][cap_atoms] */
    int32_t B, cap_atoms, cap_mol_bonds;   /* all >= 1 */
    uint8_t* text;               /* [cap_text] */
    int32_t* index;              /* [2 B + 1] */
    int32_t* work;               /* [B] */
    int64_t cap_text;            /* 1 .. 2^31 - 1 */
} abc_molblock_desc;
/* Host arithmetic only (no device is touched; of the descriptor only cap_atoms and cap_mol_bonds are read): an upper bound of ONE
 * image's text at these capacities, 0 for capacities below 1.  Derived line by line with every number at its widest: the head and the
 * counts line with both counts at max(3, digits of the capacity); cap_atoms atom lines of two 13-column coordinates (four leading
 * columns, four integer digits -- 199999 / 60 - 1 < 10000 -- and ".dddd") plus the fixed columns; cap_mol_bonds bond lines of four
 * 11-column numbers ("-2147483648"); a charge line naming every atom (index at max(4, digits), charge at 11 columns); the STY and
 * SLB lines and four lines per entry for cap_atoms implicit-H entries (entry number at the capacity's digits, atom at 11
 * columns); the end.  Not tight (a bond line of in-range rows has 13 bytes, not 45): 224 867 bytes at 512 atoms and 2048 bonds. */
int64_t abc_molblock_text_bytes(const abc_molblock_desc* d);
/* refuses null pointers, B < 1, capacities < 1, cap_text outside 1 .. 2^31 - 1, and capacities at which
 * abc_molblock_text_bytes passes 2^31 - 1 */
int abc_write_molblocks(const abc_molblock_desc* d, abc_stream_t stream);
/* sizeof(abc_molblock_desc), for a binding's mirror struct (as abc_graph_similarity_desc_size) */
int abc_molblock_desc_size(void);

/* A SMILES string for every assembled molecule, written on the device from the rows of abc_assemble_graphs, read in place
 * (csrc/smiles.hip; decode.Molecule.smiles() is the host form and the oracle; the rule with its examples: DESIGN.md section 7).
 * NOT the canonical SMILES RDKit prints: a deterministic, valid SMILES whose graph is the graph of the rows.  Wedge bonds are
 * single bonds and stereo is not written (abc_write_smiles_stereo, below, writes it); x, y, hs and the bond's source are not read.  Two launches on the stream, integers only,
 * one workgroup per image, no atomics on global memory, no allocation, no sync; deterministic.
 *   input    image b's rows, atom and bond counts clamped to their capacities: atoms (x, y, vocabulary index, charge VALUE, hs),
 *            bonds (end 1, end 2 (1-based), order 1..6, source), mol_implh k 1-based atom indices (one outside 1..n is ignored);
 *   classes  symbol: the 14-entry table of decode.ATOM_SYMBOLS (index 0 is carbon).  Order class: 5 and 6 -> 1, else the order.
 *            An atom is AROMATIC iff its symbol is one of B C N O P S Se and one of its bonds has class 4; LISTED iff mol_implh
 *            names it;
 *   token    bare ("C", "Cl", "n") iff the charge is 0, the atom is not listed and the symbol is one of B C N O P S F Cl Br I;
 *            else "[" symbol, "H" if h = 1 or "H<h>" if h >= 2, the charge ("+", "-", "+<n>", "-<n>"), "]".  An aromatic atom's
 *            symbol is in lower case ("se").  h: 1 for a listed atom (what MRV_IMPLICIT_H sets in the mol block); 0 for symbol H
 *            or |charge| > 1; else with v = floor(s2 / 2), s2 = the sum over the atom's bonds of 3 for class 4 and 2 * class
 *            otherwise, h = t - v for the smallest t >= v of the atom's valence list, 0 without such a t.  The lists, as
 *            (charge -1 | 0 | +1): B 4|3|2, C 3|4|3, N 2|3|4, O 1|2|3, F -|1|2, Si 3,5|4|3, P 2,4,6|3,5|4, S and Se 1|2,4,6|3,5,
 *            Cl, Br and I -|1|2,4,6.  The table is this library's; no agreement with RDKit's valence model is claimed;
 *   bond     between u and v: class 1 nothing, but "-" if both are aromatic; 2 "="; 3 "#"; 4 nothing if both are aromatic, else ":";
 *   walk     components in order of their lowest atom index, which is the root, joined by ".".  Depth first: visiting a gives it
 *            the next preorder rank; its neighbours are scanned in ascending atom index by a cursor that is never restarted: the
 *            tree parent and a neighbour whose edge to a already is a ring bond are skipped, a visited neighbour x makes (x, a) a
 *            ring bond OPENED at x and CLOSED at a, an unvisited one becomes the next child of a and is walked at once;
 *   digits   atoms in preorder; at each, first its closings in ascending rank of the opener, each as the bond symbol and the
 *            number, then its openings in ascending rank of the closer, each taking the lowest free number of 1..99 and written as
 *            the number alone; only then are the numbers of the closings free again.  1..9 are one digit, 10..99 "%nn";
 *   text(a)  the token of a, its digits, then "(" bond text(child) ")" for every child but the last in scan order, then bond
 *            text(last child);
 *   text     the strings of the batch back to back in image order, image b is text[offsets[b] .. offsets[b+1]) (ASCII);
 *   index    offsets[0 .. B], then status[0 .. B-1];
 *   status   ABC_MOL_EMPTY / ABC_MOL_TRUNCATED copied from mol_counts (EMPTY: length 0; zero atoms without EMPTY: the empty string,
 *            status 0); ABC_TEXT_BAD_ROW, length 0: a vocabulary index outside 0..13, a charge outside -15..15, a bond order
 *            outside 1..6, a bond end outside 1..n, both ends of a bond on one atom, a second row for an atom pair (in either
 *            orientation) -- the assembler writes none of these; ABC_TEXT_RING_LIMIT, length 0: an opening finds no free number
 *            (more than 99 ring bonds open at once); ABC_TEXT_OVERFLOW: an image is written only if the UNCLIPPED running total of
 *            the lengths through it is <= cap_text -- the first image that does not fit and every image after it have length 0 and
 *            this bit, so what is written is a prefix of the batch;
 *   work     scratch, abc_smiles_work_ints() int32: the length of every image (negative: refused), then one slice of
 *            abc_smiles_text_bytes() bytes per image -- the walk is done once, by the first launch, which leaves the image's
 *            bytes there; the second applies the prefix rule and copies. */
typedef struct abc_smiles_desc {
    const int32_t* mol_counts;   /* [B][4]                 as abc_assemble_desc.mol_counts */
    const int32_t* mol_atoms;    /* [B][cap_atoms][5] */
    const int32_t* mol_bonds;    /* [B][cap_mol_bonds][4] */
    const int32_t* mol_implh;    /* [B][cap_atoms] */
    int32_t B, cap_atoms, cap_mol_bonds;   /* B >= 1, cap_atoms 1..ABC_MAX_SMILES_ATOMS, cap_mol_bonds 1..4096 */
    uint8_t* text;               /* [cap_text] */
    int32_t* index;              /* [2 B + 1] */
    int32_t* work;               /* [abc_smiles_work_ints()] */
    int64_t cap_text;            /* 1 .. 2^31 - 1 */
} abc_smiles_desc;
/* Host arithmetic only (of the descriptor only cap_atoms and cap_mol_bonds are read): an upper bound of ONE image's text at these
 * capacities, 0 for capacities below 1.  Derived token by token with everything at its widest: every atom may stand behind a "."
 * or a "(" and a bond symbol (2), be "[" a two-letter symbol "H" and a digit, a sign and two digits "]" (9) and be followed by one
 * ")" (there are fewer brackets than atoms): 12 per atom; every bond row may be a ring bond with "%nn" at its opening and a bond
 * symbol and "%nn" at its closing: 7 per bond.  12 cap_atoms + 7 cap_mol_bonds: 20 480 bytes at 512 atoms and 2048 bonds. */
int64_t abc_smiles_text_bytes(const abc_smiles_desc* d);
/* Host arithmetic only: the int32 words of `work` (B, cap_atoms, cap_mol_bonds are read), 0 for a B or a capacity below 1 */
int64_t abc_smiles_work_ints(const abc_smiles_desc* d);
/* refuses null pointers, B < 1, capacities < 1 and cap_text outside 1 .. 2^31 - 1 (ABC_EINVAL), cap_atoms above
 * ABC_MAX_SMILES_ATOMS and cap_mol_bonds above 4096 (ABC_EUNSUPPORTED); nothing is launched then */
int abc_write_smiles(const abc_smiles_desc* d, abc_stream_t stream);
/* sizeof(abc_smiles_desc), for a binding's mirror struct (as abc_molblock_desc_size) */
int abc_smiles_desc_size(void);

/* The same text with tetrahedral stereo: the centres that the wedge rows (orders 5 and 6) and the positions decide are written as
 * "@" / "@@".  Opt-in and apart: abc_write_smiles keeps its bytes.  The same two launches (the other instantiation of the same
 * kernels), integers only, no atomics on global memory, no sync.  Everything of abc_smiles_desc holds, and the rule joins its text
 * rule (decode.Molecule.smiles(stereo=True) is the host form):
 *   frame       an atom row's (x, y) is (row, column); with z toward the viewer (row down, column right, z) is right-handed;
 *   wedge       a bond row of order 5 or 6 speaks for its END 1 alone, the narrow end, as in a mol file: seen from atom a, neighbour
 *               j has the elevation z = +1 if a row (a, j, 5) exists, -1 for (a, j, 6), 0 otherwise (also for a row (j, a, 5 | 6));
 *   candidate   an atom that is end 1 of at least one wedge row;
 *   qualified   a candidate whose symbol is not H, all of whose bonds have class 1, and whose degree d and hydrogen count h (the
 *               text rule's, for a listed atom too) are d = 4, h = 0 or d = 3, h = 1; any other candidate is UNQUALIFIED: no mark;
 *   vectors     p_j = (x_j - x_a, y_j - y_a, z_j) for every neighbour j; for d = 3 the hydrogen is a fourth neighbour at (0, 0, 0).
 *               A qualified atom is FLAT, no mark, if its own or a neighbour's x or y is outside 0..199999 (the mol block's range;
 *               every product below stays under 2^40), if a neighbour stands on the atom's own (x, y), or if T = 0;
 *   parity      T = det[p1 - p4; p2 - p4; p3 - p4] in int64 for four neighbours in some order: T > 0 says that seen from n1 the
 *               atoms n2, n3, n4 run counter-clockwise, "@"; T < 0 "@@".  The local parity s(a) is the sign of T with the
 *               neighbours in ascending atom index and the hydrogen last;
 *   mark        the text names a centre's neighbours as: the tree parent if any, the hydrogen if any, the ring numbers as written
 *               on the atom (closings, then openings), the children in scan order.  "@" iff s(a) times the sign of the permutation
 *               from the local order to that order is positive, else "@@";
 *   token       a marked atom is always bracketed: "[" symbol mark "H"? charge "]" -- "[C@@H]", "[C@]", "[N@+]" (never aromatic:
 *               all its bonds have class 1).  Nothing else of the text changes; a batch without a marked atom has the bytes of
 *               abc_write_smiles;
 *   example     atoms 1 C (20, 20), 2 N (10, 20), 3 C (25, 29), 4 O (25, 11), rows (1, 2, 5), (1, 3, 1), (1, 4, 1): d = 3, h = 1,
 *               T = det[(-10, 0, 1); (5, 9, 0); (5, -9, 0)] = -90, the text order (H, 2, 3, 4) is an odd permutation of
 *               (2, 3, 4, H): "[C@H](N)(C)O"; with order 6 "[C@@H](N)(C)O"; with the row (2, 1, 5) instead "C(N)(C)O";
 *   stereo_stats  per image (marked, flat, unqualified, wedge rows -- every row of order 5 or 6); all zeros for an image that is
 *               EMPTY or refused (BAD_ROW, RING_LIMIT).  OVERFLOW does not change it;
 *   stereo_out  optional, per atom row: 0 no candidate, +1 / -1 s(a) of a marked atom, 2 flat, 3 unqualified; every word of the
 *               image's cap_atoms is written by every launch (0 past the atom count and for an image without text).
 * Not covered: centres with a multiple bond (sulfoxides, phosphates), three-neighbour centres without a hydrogen, RDKit's special
 * cases for T-shaped drawings, stereo in the identity / similarity scores.  Double-bond marks ("/", "\"): abc_write_smiles_ez, below. */
typedef struct abc_smiles_stereo_desc {
    const int32_t* mol_counts;   /* the fields of abc_smiles_desc, in its order */
    const int32_t* mol_atoms;
    const int32_t* mol_bonds;
    const int32_t* mol_implh;
    int32_t B, cap_atoms, cap_mol_bonds;
    uint8_t* text;
    int32_t* index;
    int32_t* work;               /* [abc_smiles_stereo_work_ints()] */
    int64_t cap_text;
    int32_t* stereo_stats;       /* [B][4] */
    int32_t* stereo_out;         /* optional: [B][cap_atoms] */
} abc_smiles_stereo_desc;
/* as abc_smiles_text_bytes with a marked token at its widest: "[" two letters "@@" "H" a digit, a sign and two digits "]" (11)
 * makes 14 per atom; 14 cap_atoms + 7 cap_mol_bonds */
int64_t abc_smiles_stereo_text_bytes(const abc_smiles_stereo_desc* d);
/* as abc_smiles_work_ints, with slices of abc_smiles_stereo_text_bytes() */
int64_t abc_smiles_stereo_work_ints(const abc_smiles_stereo_desc* d);
/* the guards of abc_write_smiles, and a null stereo_stats is ABC_EINVAL; nothing is launched on a refusal */
int abc_write_smiles_stereo(const abc_smiles_stereo_desc* d, abc_stream_t stream);
/* sizeof(abc_smiles_stereo_desc), for a binding's mirror struct */
int abc_smiles_stereo_desc_size(void);

/* The same text with double-bond stereo: the single bonds at every double bond whose geometry the positions decide are written as
 * "/" or "\" in place of their (empty) symbol.  Opt-in and apart: abc_write_smiles and abc_write_smiles_stereo keep their bytes.
 * The same two launches (two more instantiations of the same kernels), integers only, no atomics on global memory, no sync.
 * Everything of abc_smiles_desc holds; with `tetrahedral` non-zero everything of abc_smiles_stereo_desc too (the two marks are
 * independent: a centre has only class-1 bonds, so it is never an end).  The rule (DESIGN.md section 7;
 * decode.Molecule.smiles(double_bonds=True) is the host form):
 *   graph       the writer's: valid rows, unique pairs, order classes (a wedge row is a class-1 bond); (x, y) is (row, column); only
 *               signs of cross products are compared, so mirror, rotation and shift change nothing;
 *   candidate   a bond row of class 2 between a and b (a the lower atom index), both C or N, each of degree 2 or 3 (one or two
 *               SUBSTITUENTS besides the partner), every substituent bond of class 1.  An atom is an end of at most one candidate;
 *   code        per bond row, the first that applies: 0 not a candidate; 3 RING: the bond lies on a cycle of ANY size (it is not a
 *               bridge); 4 TWIN: an end has two substituents of degree 1 with equal symbol, charge and listed-ness in mol_implh;
 *               2 FLAT: with d = pos(b) - pos(a) and side(e, s) = sign(d.x (pos(s).y - pos(e).y) - d.y (pos(s).x - pos(e).x)) in
 *               int64, one of the up to six atoms has x or y outside 0..199999, or some side is 0, or the two substituents of one end
 *               have the same side; else +1 (together) / -1 (opposite): the lowest-index substituents of a and of b have equal /
 *               unequal side, and the bond is MARKED;
 *   mark        every substituent bond of a marked double bond D gets a symbol where the text rule writes that bond's symbol, read
 *               as first atom, symbol, second atom: parent, child for a tree bond; closer (which bears it at its closing digit), opener
 *               for a ring bond.  "/": the second atom is above the first.  With an orientation u(D) = +1 / -1 and above(e, s) =
 *               u(D) side(e, s): "/" iff above(first, second) = +1 where the first atom is the end, iff above(second, first) = -1 where
 *               the second is.  A single bond between ends of two marked double bonds bears one symbol for both, which ties their
 *               orientations; marked double bonds are bridges, so such groups are trees and have exactly two solutions;
 *   normal form in every group the symbol written first in the text is "/" (by preorder position of the atom it is written on; at one
 *               atom the tree bond's before the closings', those in written order);
 *   example     C (10, 10), C (20, 20), C (20, 30), C (30, 40), rows (1, 2, 1), (2, 3, 2), (3, 4, 1): code -1, "C/C=C/C"; with atom 4
 *               at (10, 40) code +1, "C/C=C\C".  Stripping "/" and "\" gives the bytes written without the option;
 *   ez_stats    per image (marked, flat, ring, twin); all zeros for an image that is EMPTY or refused.  OVERFLOW does not change it;
 *   ez_out      optional, the code of every bond row; every word of the image's cap_mol_bonds is written by every launch (0 past the
 *               bond count and for an image without text).
 * The byte bound does not grow (a symbol byte per tree bond and closing is already counted).
 * Not covered: double bonds on any cycle (macrocyclic E/Z too), equivalence of an end's substituents beyond twin leaves, ends other
 * than C and N, RDKit's choice of which bonds to mark (all substituent bonds are marked), the plain canonical order
 * (abc_canonical_order_stereo is the order that reads these codes), stereo in the scores. */
typedef struct abc_smiles_ez_desc {
    const int32_t* mol_counts;   /* the fields of abc_smiles_stereo_desc, in its order */
    const int32_t* mol_atoms;
    const int32_t* mol_bonds;
    const int32_t* mol_implh;
    int32_t B, cap_atoms, cap_mol_bonds;
    uint8_t* text;
    int32_t* index;
    int32_t* work;               /* [abc_smiles_ez_work_ints()] */
    int64_t cap_text;
    int32_t* stereo_stats;       /* [B][4]: required iff tetrahedral != 0 */
    int32_t* stereo_out;         /* optional: [B][cap_atoms] (tetrahedral != 0) */
    int32_t tetrahedral;         /* non-zero: the tetrahedral marks of abc_write_smiles_stereo as well */
    int32_t* ez_stats;           /* [B][4]: marked, flat, ring, twin */
    int32_t* ez_out;             /* optional: [B][cap_mol_bonds] */
} abc_smiles_ez_desc;
/* abc_smiles_text_bytes, or abc_smiles_stereo_text_bytes with tetrahedral != 0 */
int64_t abc_smiles_ez_text_bytes(const abc_smiles_ez_desc* d);
/* as abc_smiles_work_ints, with slices of abc_smiles_ez_text_bytes() */
int64_t abc_smiles_ez_work_ints(const abc_smiles_ez_desc* d);
/* the guards of abc_write_smiles_stereo (stereo_stats only with tetrahedral != 0), and a null ez_stats is ABC_EINVAL; nothing is
 * launched on a refusal */
int abc_write_smiles_ez(const abc_smiles_ez_desc* d, abc_stream_t stream);
/* sizeof(abc_smiles_ez_desc), for a binding's mirror struct */
int abc_smiles_ez_desc_size(void);

/* Read a batch of SMILES strings into graph records on the device: the writer's inverse (csrc/smiles_read.hip; decode.parse_smiles is
 * the host form and the reference; the reading rule -- a stated subset of OpenSMILES, no claim about what RDKit accepts -- is in
 * DESIGN.md section 7, "Reading a SMILES", and its token grammar in csrc/smiles_tokens.hpp).  The records are the ones
 * raster.parse_graph fills from annotation strings, so the three scores, abc_perceive_aromatic and abc_canonical_order read them
 * unchanged: rec_atoms (0, 0, class, charge) in order of appearance, rec_bonds (i < j 0-based, order 1..4) in the order of the byte
 * that completes the bond.  Stereo marks, isotopes, hydrogen counts and atom classes are read and dropped.  One launch, one workgroup
 * of 256 threads per string with the bytes in LDS, integers only, no atomics on global memory, no sync, no allocation: capturable.
 *   text     the strings back to back; string b is the bytes text[offsets[b] .. offsets[b + 1]), every byte counts
 *   offsets  [B + 1]; a pair that is not 0 <= offsets[b] <= offsets[b + 1] <= cap_text is ABC_READ_SYNTAX for that string
 *   status   [B], exactly one abc_smiles_read_status per string, the first that holds in the enum's order; every launch writes it
 *            and rec_counts for all B strings, and every status but ABC_READ_OK leaves 0 atoms and 0 bonds (rows past the counts
 *            are unspecified)
 *   stats    optional [B][4]: bytes, atoms, bonds, ring bonds of a string that was read (bytes alone otherwise)
 *   limits   a string of more than ABC_MAX_SMILES_READ_BYTES bytes is ABC_READ_TOO_LONG: the bytes and one word or less per token
 *            live in LDS (60 KB at 4096; 8192 would pass the 64 KB a kernel gets without asking).  max_atoms and max_bonds have no
 *            upper limit: a string has fewer atoms and bonds than bytes */
#define ABC_MAX_SMILES_READ_BYTES 4096   /* a power of two: the kernel packs an atom index into 12 bits */
enum abc_smiles_read_status { ABC_READ_OK = 0, ABC_READ_EMPTY = 1, ABC_READ_TOO_LONG = 2, ABC_READ_SYNTAX = 3, ABC_READ_TRUNCATED = 4,
                              ABC_READ_DUPLICATE = 5 };
typedef struct abc_smiles_read_desc {
    const uint8_t* text;         /* [cap_text] */
    const int32_t* offsets;      /* [B + 1] */
    int32_t* rec_atoms;          /* [B][max_atoms][4] */
    int32_t* rec_bonds;          /* [B][max_bonds][3] */
    int32_t* rec_counts;         /* [2][B]: atoms, then bonds */
    int32_t B, max_atoms, max_bonds;   /* all >= 1 */
    int32_t cap_text;            /* >= 1 */
    int32_t* status;             /* [B] */
    int32_t* stats;              /* [B][4] or null */
} abc_smiles_read_desc;
/* a null descriptor, a null pointer but stats, B < 1, max_atoms < 1, max_bonds < 1 or cap_text < 1 is ABC_EINVAL; nothing is
 * launched then */
int abc_read_smiles(const abc_smiles_read_desc* d, abc_stream_t stream);
/* sizeof(abc_smiles_read_desc), for a binding's mirror struct */
int abc_smiles_read_desc_size(void);

/* ---- unet2: CBAM attention + residual (unet2.py:6-74).  See csrc/cbam.hip for the pass structure. ---- */
typedef struct abc_cbam_channel_desc { /* ChannelAttentionModule (unet2.py:6-22), one MLP evaluation per image */
    const float* partial;  /* fwd: conv stats [B*tiles_per_img][4][C] (sum,sumsq,max,min of y2); bwd: [B*tiles_per_img][C] */
    int32_t tiles_per_img, B, C, mid; double HW;
    const float* scale; const float* shift;            /* BN2 affine of this block */
    const float* w1; const float* b1; const float* w2; const float* b2; /* shared_MLP.0 / .2 */
    float* ca; float* avgz; float* maxz; float* hid_avg; float* hid_max; /* [B][C], [B][C], [B][C], [B][mid] x2 */
    float* dw1; float* db1; float* dw2; float* db2; float* d_avgz; float* d_maxz; /* backward outputs */
    float* work;           /* backward scratch, B * (C + 2 mid) floats */
    /* forward outputs for the backward of AdaptiveMaxPool2d(1) (unet2.py:10,20): ext[n][c] = the extreme RAW value of y2 whose BN image is
     * max(z) (max of y2 for a positive BN scale, min for a negative one); first[n][c] is reset to INT32_MAX here and lowered by
     * abc_cbam_spatial_stats to the first pixel (row-major) holding that value -- the one torch routes the gradient to */
    float* ext; int32_t* first;
} abc_cbam_channel_desc;
int abc_cbam_channel_fwd(const abc_cbam_channel_desc* d, abc_stream_t stream);
int abc_cbam_channel_bwd(const abc_cbam_channel_desc* d, abc_stream_t stream);
/* abc_cbam_channel_bwd + the pending reduction of c7->dw_partial into c7->dw7 / c7->db7 (see abc_cbam_conv7_bwd_partial) */
struct abc_cbam_conv7_desc;
int abc_cbam_channel_bwd_c7(const abc_cbam_channel_desc* d, const struct abc_cbam_conv7_desc* c7, abc_stream_t stream);

typedef struct abc_cbam_pix_desc { /* per-pixel passes of SpatialAttentionModule / CBAM / residual (unet2.py:24-74) */
    const void* y; int32_t ld_y, cy_off;               /* raw second-conv output y2 */
    const float* scale; const float* shift; const float* mean; const float* invstd;
    const float* ca; const float* maxz; const float* d_avgz; const float* d_maxz;
    const float* sa; float* st; int32_t* amax; float* du; const float* dst;
    const void* res; int32_t ld_res, cres_off, res_pool; /* residual r (res_pool: 2x2 max of a 2x tensor) */
    void* out; int32_t ld_out, cout_off;               /* block output relu(sa*ca*z + r) */
    const void* d_same; int32_t ld_same, csame_off;    /* gradient sources wrt `out` */
    const void* d_pool; int32_t ld_pool, cpool_off;
    void* g; int32_t ld_g;                             /* dOut*[out>0] (the residual branch's gradient) */
    void* dz; int32_t ld_dz;                           /* d_o1, then d_z in place */
    float* partial;
    int32_t dtype, B, H, W, C;
    const float* ext; int32_t* first;  /* see abc_cbam_channel_desc: spatial_stats lowers first[n][c], bwd3 adds d_maxz at that pixel only */
} abc_cbam_pix_desc;
int abc_cbam_spatial_stats(const abc_cbam_pix_desc* d, abc_stream_t stream); /* y,ca -> st[B,H,W,2], amax */
int abc_cbam_apply_fwd(const abc_cbam_pix_desc* d, abc_stream_t stream);     /* -> out */
int abc_cbam_bwd1(const abc_cbam_pix_desc* d, abc_stream_t stream);          /* -> g, du */
int abc_cbam_bwd2_blocks(const abc_cbam_pix_desc* d);                        /* workgroups per image */
int abc_cbam_bwd2(const abc_cbam_pix_desc* d, abc_stream_t stream);          /* -> dz = d_o1, partial [B][blocks][C] */
int abc_cbam_bwd3_blocks(const abc_cbam_pix_desc* d);
int abc_cbam_bwd3(const abc_cbam_pix_desc* d, abc_stream_t stream);          /* dz -> d_z in place, BN partial [blocks][2][C] */

typedef struct abc_cbam_conv7_desc { /* SpatialAttentionModule.conv2d 7x7 (2->1) + sigmoid (unet2.py:27,34) */
    const float* st; const float* w7; const float* b7; float* sa;
    const float* du; float* dst; float* dw_partial; float* dw7; float* db7; /* backward */
    int32_t B, H, W;
} abc_cbam_conv7_desc;
int abc_cbam_conv7_fwd(const abc_cbam_conv7_desc* d, abc_stream_t stream);
int abc_cbam_conv7_blocks(const abc_cbam_conv7_desc* d); /* dw_partial = [blocks][99] */
int abc_cbam_conv7_bwd(const abc_cbam_conv7_desc* d, abc_stream_t stream);
/* the same without the reduction of dw_partial: abc_cbam_channel_bwd_c7 of the same block performs it inside its first launch
 * (the reduction is independent of the channel attention's backward and was a ~5 us launch of its own, 13 per step of unet2.py) */
int abc_cbam_conv7_bwd_partial(const abc_cbam_conv7_desc* d, abc_stream_t stream);

/* dst[.., cdst_off + c] += src[.., csrc_off + c] (identity residual gradient, unet2.py:62) */
int abc_add_into(void* dst, int32_t ld_dst, int32_t cdst_off, const void* src, int32_t ld_src, int32_t csrc_off, int32_t C,
                 int64_t npix, int32_t dtype, abc_stream_t stream);

/* nn.MaxPool2d(2) of an activated tensor (unet.py:30), materialised once: out[b][y][x][c] = max over the 2x2 window
 * of act(src[b][2y+dy][2x+dx][c_off + c]) (src->pool is ignored: src is read at full resolution).  The encoder's
 * first convolution of every level and its weight gradient then read a plain NHWC tensor on their prefetch paths
 * instead of pooling on load twice. */
int abc_pool_act(const abc_act_src* src, int32_t dtype_in, int32_t c_off, int32_t C, int32_t B, void* out, int32_t dtype_out,
                 int32_t ld_out, abc_stream_t stream);

/* layout conversion helpers (multi-channel NCHW input images -> NHWC) */
int abc_nhwc_to_nchw_f32(const float* src, int32_t ld, int32_t c_off, int32_t C, int32_t B, int32_t H, int32_t W,
                         float* dst, abc_stream_t stream);
int abc_nchw_to_nhwc_f32(const float* src, int32_t C, int32_t B, int32_t H, int32_t W, float* dst, int32_t ld,
                         int32_t c_off, abc_stream_t stream);
int abc_fill_f32(float* p, float v, int64_t n, abc_stream_t stream);
/* dst = srcs[0][0:counts[0]] ++ srcs[1][0:counts[1]] ++ ... (n <= 16 device arrays; `srcs` / `counts` are HOST arrays read at
 * call time): the eight heads' conv1 biases (unet.py:66) side by side for the one merged convolution */
int abc_concat_f32(const float* const* srcs, const int32_t* counts, int32_t n, float* dst, abc_stream_t stream);
/* *p += inc (one thread): the per-step dropout salt */
int abc_counter_add_u32(uint32_t* p, uint32_t inc, abc_stream_t stream);

/* The bf16 wire format of the data-parallel gradient exchange (multi_gpu_train.py:44-52,114-119).  bf16(x) is
 * round-to-nearest-even on the f32 bit pattern u: (u + 0x7FFF + ((u >> 16) & 1)) >> 16; any NaN becomes a quiet NaN (never Inf),
 * +-0 and +-Inf are kept, f32 subnormals are rounded (not flushed), finite values above the largest bf16 become Inf.
 *   abc_grad_pack_bf16:   dst[i] = bf16(src[i]), i in [0, n)
 *   abc_grad_reduce_bf16: recv is [W][n] bf16, 1 <= W <= 64; acc = f32(recv[0][i]), then acc = acc + f32(recv[q][i]) for
 *                         q = 1 .. W-1 in that order (plain f32 adds), dst[i] = bf16(acc)
 *   abc_grad_unpack_bf16: dst[i] = f32(src[i]) (exact)
 * Any n >= 1 and any element-aligned pointers (f32: 4 bytes, bf16: 2); source and destination must not overlap.  One launch
 * each, no allocation, no synchronisation. */
int abc_grad_pack_bf16(const float* src, void* dst, int64_t n, abc_stream_t stream);
int abc_grad_reduce_bf16(const void* recv, void* dst, int32_t W, int64_t n, abc_stream_t stream);
int abc_grad_unpack_bf16(const void* src, float* dst, int64_t n, abc_stream_t stream);

/* sizeof(descriptor #which) in declaration order (abc_act_src = 0 ... abc_nms_desc = 12, abc_cbam_channel_desc = 13, abc_cbam_pix_desc = 14, abc_cbam_conv7_desc = 15, abc_metrics_desc = 16, abc_extract_desc = 17, abc_raster_desc = 18, abc_heads_fused_desc = 19, abc_heads_epi = 20, abc_convt_desc = 21, abc_loss_scale_desc = 22, abc_adam_seg = 23, abc_adam_class = 24, abc_adam_multi_desc = 25, abc_image_desc = 26, abc_assemble_desc = 27):
 * lets a foreign-language binding check its mirror structs at load time */
int abc_sizeof(int which);
const char* abc_last_error(void);
int abc_version(void);
/* Leave `n` (rounded up to a multiple of 4; 0 <= n <= 128) of the 256 compute units out of the PERSISTENT convolution grids
 * (the launches sized to 2 or 3 workgroups per CU): process-wide, read when a launch sizes its grid -- set it before a plan is
 * built or captured.  For the data-parallel step (multi_gpu_train.py:44-53 / DDP's NCCL kernels beside backward): two 256-VGPR
 * workgroups per CU leave no registers for a communication kernel, which would wait for a persistent workgroup to drain. */
int abc_set_reserved_cus(int32_t n);
int abc_get_reserved_cus(void);

#ifdef __cplusplus
}
#endif
#endif
