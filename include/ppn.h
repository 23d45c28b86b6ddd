/*
 * libppn -- MI355X (gfx950) native Pose Proposal Network hot path, C ABI.
 *
 * The reference (noirmist/Pytorch_Pose_Proposal_Network) is 100 % Python and has no FFI;
 * its call surface for this path is
 *     PoseProposalNet.forward            model.py:104-136   (conv/BN/act stack)
 *     rt_test.inference                  rt_test.py:87-147  (normalise, forward, slice, decode)
 *     datatest.get_humans_by_feature     datatest.py:74-132 (decode + root NMS + limb parse)
 *     datatest.non_maximum_suppression   datatest.py:134-160
 *     PPNLoss.forward + loss.backward()  main.py:125-216, 664-683 (fused loss forward + gradient)
 *     train()                            main.py:623-777   (train-mode BN, conv gradients, GradNorm task weights,
 *                                                           Adam; see "Training building blocks" below)
 *     KeypointsDataset target encoding   dataset.py:96-185
 * The entry points below are what a ctypes binding for those functions binds
 * (INTEGRATION.md shows the stub).  Conventions:
 *   - every function returns 0 on success, a negative PPN_E_* code on error;
 *     ppn_last_error() returns a thread-local message.  No C++ exception crosses the ABI.
 *   - all tensor arguments are BORROWED raw device pointers (PyTorch-ROCm owns the memory);
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     every launch is asynchronous on that stream; nothing here synchronises or allocates,
 *     except ppn_plan_create/ppn_plan_destroy (host memory, optional hipGraph).
 *   - not thread-safe per handle (the reference is single-threaded).
 */
#ifndef PPN_H
#define PPN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPN_OK 0
#define PPN_E_INVALID (-1)   /* bad argument / unsupported shape */
#define PPN_E_HIP (-2)       /* a HIP runtime call failed */
#define PPN_E_UNSUPPORTED (-3)

#define PPN_MAX_EDGES 32
#define PPN_MAX_KP 32

const char* ppn_last_error(void);
int ppn_version(void);

/* ------------------------------------------------------------------------------------------
 * Decode: grid-cell decode + root-box NMS + greedy limb parse on the DEVICE head tensor.
 * Replaces datatest.py:74-132 (get_humans_by_feature) incl. the head slicing and
 * delta = resp*conf of rt_test.py:106-130; bit-exact on every index it returns.
 * ---------------------------------------------------------------------------------------- */
typedef struct ppn_decode_cfg {
    int32_t K, E;                 /* keypoints (18), edges (17)                config.py:64-65   */
    int32_t sH, sW;               /* local limb window (21,21)                 rt_test.py:58     */
    int32_t H, W;                 /* output grid (24,24)                       datatest.py:54    */
    int32_t inH, inW;             /* network input size (384,384)              datatest.py:53    */
    float det_thr;                /* 0.15  rt_test.py:133                                        */
    float nms_thr;                /* 0.3   datatest.py:94                                        */
    int32_t min_kp;               /* 1     datatest.py:74                                        */
    int32_t max_humans;           /* rows per image in the output buffers (<= H*W)               */
    int32_t edge_src[PPN_MAX_EDGES];   /* EDGES[e][0]                          config.py:65      */
    int32_t edge_dst[PPN_MAX_EDGES];   /* EDGES[e][1]                                            */
    int32_t edge_order[PPN_MAX_EDGES]; /* edges parent-before-child (tree form of DIRECTED_GRAPHS,
                                          config.py:67-80)                                      */
} ppn_decode_cfg;

/* Bytes of device scratch ppn_decode needs for `batch` images (limb arg-max map + the root-NMS survivor lists that
 * the first workgroup per image of the arg-max launch leaves for the parse kernel). */
size_t ppn_decode_workspace_bytes(const ppn_decode_cfg* cfg, int32_t batch);

/*
 * head       f32 [batch, 6K + E*sH*sW, H, W]  sigmoid outputs, NCHW contiguous (model.py:136)
 * workspace  >= ppn_decode_workspace_bytes()
 * out_count  i32 [batch]                          humans kept per image (before max_humans clamp)
 * out_kp_cell  i32 [batch, max_humans, K]         row-major cell h*W+w of each accepted keypoint, -1 absent
 * out_limb_arg i32 [batch, max_humans, E]         arg-max index sh*sW+sw of each evaluated limb, -1 otherwise
 * out_bbox   f32 [batch, max_humans, K, 4]        (ymin,xmin,ymax,xmax)  datatest.py:80-86
 * out_score  f32 [batch, max_humans, K]           delta = resp*conf of accepted keypoints
 * Humans are ordered by descending root score (datatest.py:103,139); equal scores by ascending cell.
 * Grids of up to H*W <= 704 cells (for K = 18, E = 17; 22 x 32 is one of the largest): the parse workgroup keeps its
 * tables in 160 KB of LDS.  A larger grid returns PPN_E_UNSUPPORTED before anything is launched, here and in
 * ppn_decode_fused / ppn_decode_fused_ws; ppn_limb_argmax alone has no such limit.
 */
int ppn_decode(const ppn_decode_cfg* cfg, const float* head, int32_t batch, void* workspace,
               int32_t* out_count, int32_t* out_kp_cell, int32_t* out_limb_arg, float* out_bbox,
               float* out_score, void* stream);

/* ppn_decode for the fused head conv: `unary` f32 [batch, 6K, H, W] and `keys` u64 [batch, E, H, W] as written
 * by ppn_conv2d_fused with argmax_keys set.  Same outputs, bit-identical to ppn_decode on the full head. */
int ppn_decode_fused(const ppn_decode_cfg* cfg, const float* unary, const uint64_t* keys, int32_t batch,
                     int32_t* out_count, int32_t* out_kp_cell, int32_t* out_limb_arg, float* out_bbox,
                     float* out_score, void* stream);

/* ppn_decode_fused with a device workspace (>= ppn_decode_fused_workspace_bytes, 16-byte aligned): the O(n^2) pairwise-IoU
 * bit matrix of every image's root candidates (datatest.py:134-160 inside get_humans_by_feature, :87-95) is then computed
 * by a launch of 8 workgroups per image in front of the per-image parse workgroup, which only runs the greedy order on it
 * (dense heads: ~490 of 576 cells are candidates on the benchmark's synthetic checkpoint).  Images with fewer than 128
 * candidates keep the single-workgroup form.  Same results, bit for bit. */
size_t ppn_decode_fused_workspace_bytes(const ppn_decode_cfg* cfg, int32_t batch);
int ppn_decode_fused_ws(const ppn_decode_cfg* cfg, const float* unary, const uint64_t* keys, int32_t batch, void* workspace,
                        int32_t* out_count, int32_t* out_kp_cell, int32_t* out_limb_arg, float* out_bbox,
                        float* out_score, void* stream);

/* First half of ppn_decode on its own (the HBM-bound kernel): dense first-index arg-max over the
 * sH*sW limb window for every (image, edge, cell).  out_arg i32 [batch, E, H, W]. */
int ppn_limb_argmax(const ppn_decode_cfg* cfg, const float* head, int32_t batch, int32_t* out_arg,
                    void* stream);

/*
 * datatest.py:134-160 non_maximum_suppression.  bbox f32 [n,4] (ymin,xmin,ymax,xmax) on device,
 * score f32 [n] or NULL, limit <= 0 means None.  out_sel i32 [n] receives the selected indices in the
 * reference's order (descending score when score is given; equal scores, -0.0 and +0.0 included, by ascending
 * index), out_count i32 [1].  n <= 998: the pairwise bit matrix and the sort live in 160 KB of LDS, and a larger n
 * returns PPN_E_UNSUPPORTED before anything is launched.
 */
int ppn_nms(const float* bbox, const float* score, int32_t n, float thresh, int32_t limit, int32_t* out_sel,
            int32_t* out_count, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training loss (forward + backward), replaces PPNLoss.forward + autograd through it (main.py:125-216, 664-683).
 * ---------------------------------------------------------------------------------------- */
typedef struct ppn_loss_cfg {
    int32_t K, E, sH, sW, H, W, inH, inW;   /* as in ppn_decode_cfg */
} ppn_loss_cfg;

size_t ppn_loss_workspace_bytes(const ppn_loss_cfg* cfg, int32_t batch);

/*
 * head        f32 [B, 6K+E*sH*sW, H, W]   feature_map (sigmoid outputs)
 * delta, weight, tx_half, ty_half, tx, ty, tw, th   f32 [B,K,H,W];  weight_ij, te  f32 [B,E,sH,sW,H,W]
 *             (the CustomBatch fields of dataset.py:233-248, argument order of main.py:180)
 * coeff       HOST pointer to 5 floats c_i (read at call time); may be NULL when grad_head is NULL
 * losses      f32 [5] device: loss_resp, loss_iou, loss_coor, loss_size, loss_limb (each summed over the
 *             non-batch dims, then mean over the batch -- main.py:199-214); bitwise reproducible
 * grad_head   f32 like head or NULL: d(sum_i c_i L_i)/d(head); with c_i = w_i/5 this is the backward of
 *             main.py:668-683, with a one-hot c the per-loss gradient the GradNorm step needs (main.py:704-708)
 */
int ppn_loss_fwd_bwd(const ppn_loss_cfg* cfg, const float* head, int32_t batch, const float* delta,
                     const float* weight, const float* weight_ij, const float* tx_half, const float* ty_half,
                     const float* tx, const float* ty, const float* tw, const float* th, const float* te,
                     const float* coeff, float* losses, float* grad_head, void* workspace, void* stream);

/*
 * ppn_loss_fwd_bwd with the five coefficients read on the DEVICE when the kernels run: c_i = coeff_dev[i] / coeff_div
 * (main.py:668 `loss = sum_i w_i l_i / 5` with the task weights optimizerR.step() left on the device, main.py:761-777).
 * The host passes no value, so it can enqueue an iteration before the previous one has finished.
 */
int ppn_loss_fwd_bwd_dev(const ppn_loss_cfg* cfg, const float* head, int32_t batch, const float* delta,
                         const float* weight, const float* weight_ij, const float* tx_half, const float* ty_half,
                         const float* tx, const float* ty, const float* tw, const float* th, const float* te,
                         const float* coeff_dev, float coeff_div, float* losses, float* grad_head, void* workspace,
                         void* stream);

/*
 * ppn_loss_fwd_bwd_dev and ppn_head_grad in one pass over the head: the five losses and, instead of d loss / d head in
 * the head layout, the gradient w.r.t. conv3's LOGITS in the layout the convolutions' backward reads:
 *   dz     `dtype` (PPN_F32 / PPN_BF16) [B][H*W][cpad] NHWC = g * s(1-s), channels >= 6K + E*sH*sW zero; cpad % 64 == 0
 *   dbsum  f32 [B][ceil(H*W/64)][cpad]: per-block cell sums of dz; summed over the first two axes = d loss / d conv3.bias
 *   grad_unary  f32 scratch [B][6K][H*W] (the unary channels' d loss / d head)
 * workspace >= ppn_loss_dz_workspace_bytes(cfg, batch, cpad).  Saves the f32 head-layout gradient (17 MB per image
 * written once and read twice).  loss_limb is summed per 64 x 64 block and then in a fixed order (reproducible; it
 * differs from ppn_loss_fwd_bwd's value in the last bits).
 */
size_t ppn_loss_dz_workspace_bytes(const ppn_loss_cfg* cfg, int32_t batch, int32_t cpad);
int ppn_loss_fwd_bwd_dz(const ppn_loss_cfg* cfg, const float* head, int32_t batch, const float* delta,
                        const float* weight, const float* weight_ij, const float* tx_half, const float* ty_half,
                        const float* tx, const float* ty, const float* tw, const float* th, const float* te,
                        const float* coeff_dev, float coeff_div, float* losses, float* grad_unary, int32_t dtype,
                        int32_t cpad, void* dz, float* dbsum, void* workspace, void* stream);
/* ... with the limb targets as ppn_encode_targets_c's compact bytes instead of weight_ij / te (bit-identical results) */
int ppn_loss_fwd_bwd_dz_c(const ppn_loss_cfg* cfg, const float* head, int32_t batch, const float* delta,
                          const float* weight, const uint8_t* limb_compact, const float* tx_half, const float* ty_half,
                          const float* tx, const float* ty, const float* tw, const float* th, const float* coeff_dev,
                          float coeff_div, float* losses, float* grad_unary, int32_t dtype, int32_t cpad, void* dz,
                          float* dbsum, void* workspace, void* stream);

/*
 * Training-target encoder (dataset.py:96-185) on the device: person lists -> the ten target tensors of
 * ppn_loss_fwd_bwd, bit-exact with the host encoder.  Replaces the per-sample host encoding + 2 x 17.3 MB/sample
 * H2D of main.py:649-661.
 *   edges    HOST i32 [E][2]  (src, dst keypoint of every limb, config.py:44-62)
 *   people   f32 [B][pmax][5 + 2*(K-1)] device: cx, cy, w, h (instance box, centre format), size (side of a part box,
 *            pixels), then x, y of keypoints 1..K-1 in input pixels
 *   visible  i32 [B][pmax] device: bit k-1 set = keypoint k is labeled;  count i32 [B]: people per image (<= pmax)
 * People are applied in list order (a later person overwrites a grid cell an earlier one claimed).
 */
int ppn_encode_targets(const ppn_loss_cfg* cfg, const int32_t* edges, const float* people, const int32_t* visible,
                       const int32_t* count, int32_t batch, int32_t pmax, float* delta, float* weight,
                       float* weight_ij, float* tx_half, float* ty_half, float* tx, float* ty, float* tw, float* th,
                       float* te, void* stream);
/* ... and, besides the ten f32 tensors, limb_compact u8 [B][E][sH][sW][H][W]: te and weight_ij in two bits per element
 * (bit 0: te = 1, bit 1: weight_ij = 1; weight_ij is 1 or 0.0005 for delta maps of 0 / 1, which is what this encoder
 * writes).  ppn_loss_fwd_bwd_dz_c and ppn_loss_limb_dual_nhwc_c -- the two kernels of a training iteration that stream the
 * limb targets -- read it instead of the two f32 tensors (1 byte instead of 8 per element: 1.1 GB less HBM traffic per
 * kernel at batch 32), with bit-identical results. */
int ppn_encode_targets_c(const ppn_loss_cfg* cfg, const int32_t* edges, const float* people, const int32_t* visible,
                         const int32_t* count, int32_t batch, int32_t pmax, float* delta, float* weight,
                         float* weight_ij, float* tx_half, float* ty_half, float* tx, float* ty, float* tw, float* th,
                         float* te, uint8_t* limb_compact, void* stream);

/*
 * Gradient of the four unary losses only: d(sum_{i<4} coeff4_i L_i)/d(head[:, 0:6K]) into grad_head (head layout;
 * the limb channels are not touched, no loss values are produced).  The GradNorm probe passes for losses 0..3
 * (main.py:704-707) need nothing else: their gradients live in the first 6K of the 7605 channels.  coeff4 is a
 * HOST pointer to 4 floats.
 */
int ppn_loss_unary_bwd(const ppn_loss_cfg* cfg, const float* head, int32_t batch, const float* delta,
                       const float* weight, const float* tx_half, const float* ty_half, const float* tx,
                       const float* ty, const float* tw, const float* th, const float* coeff4, float* grad_head,
                       void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Convolution stack: one fused launch per convolution of PoseProposalNet.forward
 * (model.py:104-136, drn.py:42-57,77-97,192-202).
 *   acc  = conv(src, weight)                        implicit GEMM on MFMA, NHWC activations
 *   v    = act1(acc * scale1 + shift1)              folded conv-bias / eval-mode BN + ReLU/LReLU/sigmoid
 *   v   += residual                                 (optional)
 *   out_raw = v                                     (optional)
 *   out_act = act2(v * scale2 + shift2)             (optional) pre-activation of the consumer block
 * ---------------------------------------------------------------------------------------- */
enum { PPN_ACT_NONE = 0, PPN_ACT_RELU = 1, PPN_ACT_LRELU = 2, PPN_ACT_SIGMOID = 3 };
/* PPN_F16: IEEE half operands (v_mfma_f32_16x16x32_f16: the bf16 MFMA rate, 3 more mantissa bits), f32 accumulation,
 * f32 head -- inference only (the conv stack, ppn_plan_add_stem012, ppn_pack_weight); the training entry points take
 * PPN_F32 / PPN_BF16. */
/* PPN_F16X3 (round 4): split-precision inference mode for the convolutions with cin % 64 == 0.  Activations are NHWC
 * half PAIRS [pixel][hi(C) | lo'(C)] (hi = half(v), lo' = half((v - hi) * 2^11)), weights are packed by
 * ppn_pack_weight_x3 as three half copies per 64-channel slab, and the K loop accumulates a_hi w_hi + a_hi w_lo + a_lo w_hi
 * in f32 on v_mfma_f32_16x16x32_f16: 22-bit operands at a third of the f16 MFMA rate.  Meets the 1e-4 head tolerance
 * (tests/test_x3_gpu.py); the layers with cin < 64 (stem, the first block's stride-2 convs) run as PPN_F32 and their
 * outputs are converted by ppn_split_f16x3. */
enum { PPN_F32 = 0, PPN_BF16 = 1, PPN_F16 = 2, PPN_F16X3 = 3 };

typedef struct ppn_conv_desc {
    int32_t dtype;               /* PPN_F32 (exact-f32 MFMA, parity mode), PPN_BF16 or PPN_F16 (16-bit MFMA, f32 accumulate) */
    int32_t batch, in_h, in_w, cin;
    int32_t out_h, out_w, cout;
    int32_t ksize, stride, dilation, pad;
    int32_t k_total;             /* padded GEMM depth of the packed weight rows (multiple of the K step) */
    int32_t cout_pad;            /* rows in the packed weight matrix (multiple of the channel tile)  */
    int32_t act1, act2;
    int32_t out_nchw_f32;        /* 1: out_raw is f32 NCHW [B,cout,H,W] (the head, model.py:136)     */
    const void* src;             /* NHWC [B,in_h,in_w,cin] dtype                                      */
    const void* weight;          /* packed [cout_pad][k_total] dtype, depth order per ppn_conv_tiling  */
    const float* scale1;         /* [cout] or NULL (=1)                                               */
    const float* shift1;         /* [cout] or NULL (=0)                                               */
    const void* residual;        /* NHWC [B,out_h,out_w,cout] dtype or NULL                           */
    void* out_raw;               /* NHWC dtype (or NCHW f32) or NULL                                  */
    const float* scale2;         /* [cout] or NULL                                                    */
    const float* shift2;         /* [cout] or NULL                                                    */
    void* out_act;               /* NHWC dtype or NULL                                                */
    const void* zero_page;       /* >= 256 B of zeros on device (padding source)                      */
    /* Fused decode front end for the head conv (out_nchw_f32 = 1): when argmax_keys != NULL the epilogue also
     * writes the first `unary_channels` (= 6K) sigmoid outputs to `unary_out` f32 [B,unary_channels,H,W] and folds
     * every limb channel into `argmax_keys` u64 [B,E,H,W] (key = value bits << 32 | ~window index; the caller
     * zeroes the buffer before the launch, see ppn_plan_add_memset).  out_raw may then be NULL: the 17.5 MB/image
     * head tensor is never written (rt_test.py:109-120 copies it to the host instead).  ppn_decode_fused consumes
     * the two buffers. */
    /* Fused 1x1 projection shortcut (BasicBlock.downsample, drn.py:53-54): when src2 != NULL the GEMM depth is
     * extended by cin2 values gathered from src2 NHWC [B,in2_h,in2_w,cin2] at (oy*stride2, ox*stride2); the packed
     * weight rows carry [main conv | shortcut 1x1 weights pre-multiplied by the shortcut BN scale] and shift1
     * carries the shortcut BN shift, so  out = conv(src) + bn_ds(conv1x1(src2))  costs no extra launch and no
     * residual tensor.  k_total = k_main + cin2, both multiples of the K step; scale1 must be NULL. */
    const void* src2;
    int32_t in2_h, in2_w, cin2, stride2;
    float* unary_out;
    uint64_t* argmax_keys;
    int32_t unary_channels;      /* 6K = 108                                                          */
    int32_t limb_window;         /* sH*sW = 441                                                       */
    /* Output-pixel range of this launch, in the flattened [batch*out_h*out_w] order: pixels m_begin .. m_begin +
     * m_count - 1 are computed, the rest of the output tensors is left untouched.  m_count = 0 (default): the whole
     * tensor (under tile policy 2 ppn_conv2d_fused then cuts the range itself where ppn_conv_split says so; a plan
     * lists the two ranges as separate entries so that each launch is timed and named). */
    int32_t m_begin, m_count;
    /* Edge-aligned limb part of the head conv (the fast fused path): limb_edge_pad = 448 (the only size built: windows of
     * 433..448 values, e.g. 21 x 21 = 441; any other window is PPN_E_UNSUPPORTED) says that `weight`, `scale1` and `shift1` hold ONLY the limb channels, edge e's
     * window in rows [e * limb_edge_pad, e * limb_edge_pad + limb_window) and padding after it (cout = E * limb_window,
     * cout_pad = E * limb_edge_pad).  One workgroup then owns a whole window of 128 cells, reduces its arg-max on the
     * accumulators and STORES argmax_keys u64 [B,E,H,W] (same key format; no atomics, the buffer need not be zeroed).
     * out_raw, unary_out must be NULL and unary_channels 0: the 6K unary channels are an ordinary NCHW launch of their
     * own (cout = 6K, out_raw = the compact unary tensor).  0 (default): the chunked epilogue with atomicMax keys. */
    int32_t limb_edge_pad;
    /* PPN_CONV_* bits, 0 by default.  Carried by the descriptor (and therefore by each plan entry), never process-wide:
     * PPN_CONV_NO_FILTER_BANK routes a 64 -> 64 3x3 stride-1 convolution of the 16-bit modes through the generic
     * implicit-GEMM kernel instead of the register-resident filter-bank kernel (csrc/conv64.hip), whose workgroups own a
     * CU's whole LDS and register file -- the choice of a plan that shares the GPU with other lanes' plans
     * (rt.MultiLaneInference).  Results are bit-identical either way. */
    int32_t flags;
    /* Prefetch hint (round 5; large-tile kernel only, ignored elsewhere): `prefetch_bytes` bytes at `prefetch` -- the packed
     * weights of the NEXT launch of a plan -- are touched once (one dword per 128-byte line, shared out over the workgroups)
     * before this launch's epilogue, which puts them into the Infinity Cache.  In the forward pass a layer's weights were
     * last read one whole pass (> 1 GB of traffic) ago, so its first round of workgroups otherwise fetches every K step's
     * weight slab from HBM in lockstep (profiles/r05/cold_operands.txt: 80 vs 100 us on the 24 x 24 512-wide layers).
     * Results do not depend on it.  NULL / 0: none. */
    const void* prefetch;
    int64_t prefetch_bytes;
    /* Train-mode BatchNorm statistics from this launch's epilogue (round 5; large-tile kernel, 16-bit single-output NHWC launches
     * without a residual -- elsewhere the launch runs as usual and reports 0 tiles).  Each pixel tile folds, per output channel,
     * two sums over ITS pixels of the values it stores (v, after rounding to the tensor's type) and writes them as f64 pairs
     * stats_partial[(tile * cout + c) * 2 + {0, 1}] -- the layout ppn_bn_train_fwd / ppn_bn_train_bwd fold their own reduction
     * pass from, so that pass is skipped (ppn_bn_desc.stats_blocks):
     *   stats_mode 1 (the convolution that FEEDS a BatchNorm, drn.py:47-63):   { sum v, sum v^2 }
     *   stats_mode 2 (the input-gradient convolution whose result is dy of a BatchNorm + activation over stats_x):
     *                { sum g, sum g * xhat },  g = v * act'(x * gamma * rstd + beta - mean * gamma * rstd),  xhat = (x - mean) * rstd
     * *stats_tiles (HOST int) receives the number of pixel tiles written, 0 if this launch does not produce statistics. */
    void* stats_partial;
    int32_t stats_mode, stats_act;
    const void* stats_x;                       /* mode 2: the BatchNorm's input, NHWC like this launch's output */
    const float *stats_gamma, *stats_beta, *stats_mean, *stats_rstd;
    int32_t* stats_tiles;
    /* Split-K workspace (flags & PPN_CONV_SPLIT_K, csrc/conv_splitk.hip): `splitk_ws_bytes` bytes of device memory, 16-byte
     * aligned, at least what ppn_conv_splitk_workspace reports for this descriptor.  Scratch: every byte the launch reads it
     * has written first, so the buffer needs no initialisation and one buffer may serve every launch of a stream in turn. */
    void* splitk_ws;
    int64_t splitk_ws_bytes;
} ppn_conv_desc;
#define PPN_CONV_NO_FILTER_BANK 1
/* PPN_CONV_SHARED_GPU: this launch runs beside other streams' launches (rt.MultiLaneInference): the tile chooser then
 * leaves out the tiles that only shorten a LONE launch by filling every CU with smaller, less efficient workgroups (the
 * 144 x 256 tile of the 24 x 24 layers: -11 % in sequence, +19 % CU-time, -3.5 % images/s with three lanes). */
#define PPN_CONV_SHARED_GPU 2
/* PPN_CONV_OUT_BF16: a PPN_F16 launch (large-tile kernel, NHWC) stores out_raw / out_act as bf16 -- the last launch of an
 * IEEE-half PREFIX in front of a bf16 trunk.  The bf16 mode runs the stem and layer3-4 (6.9 % of DRN-D-22's FLOPs) in half
 * since round 4: same kernels, same rate, and the rounding noise injected there is what every later layer amplifies. */
#define PPN_CONV_OUT_BF16 4
/* PPN_CONV_X3_PLAIN_OUT: a PPN_F16X3 launch stores out_raw / out_act as plain IEEE-half NHWC tensors [pixel][Cout] instead of
 * half pairs -- the last launch of an exact (f32 + float16x3) PREFIX in front of a float16 trunk
 * (PoseProposalNet(compute_dtype="float16", exact_prefix=3): stem + layer3 exact, 251 of the reference's 260 people). */
#define PPN_CONV_X3_PLAIN_OUT 8
/* PPN_CONV_SPLIT_K: run this convolution as a split-K pair of launches (csrc/conv_splitk.hip) -- for launches whose
 * pixels x channels fill a fraction of the GPU (batch 1-4 inference): the GEMM depth is cut into slabs of 512 values (a
 * function of k_total alone), pixel tiles x channel tiles x slabs workgroups write f32 partial tiles to `splitk_ws` with plain
 * stores, and a second launch sums them in slab order and applies the epilogue above.  Deterministic, and image i of a batch
 * gets the bits it gets alone.  Scope: PPN_F32 / PPN_BF16 / PPN_F16, cin a multiple of the K step, ksize 1 or 3, NHWC outputs
 * (PPN_CONV_OUT_BF16 included), whole-tensor launches, cout_pad a multiple of 64.  PPN_F16X3, src2, the NCHW head / arg-max /
 * limb_edge_pad modes and stats_mode != 0 return PPN_E_UNSUPPORTED, a NULL or too small workspace PPN_E_INVALID; nothing is
 * launched then and there is no fallback to the one-launch kernels.  The prefetch hint is ignored. */
#define PPN_CONV_SPLIT_K 16

/* GEMM-depth step / channel tile the packer must pad to for a conv of this shape and dtype, and the order of
 * the GEMM depth index in the packed weight rows:
 *   k_order 0:  k = (ky*ksize + kx)*cin + ci                      (tap-major)
 *   k_order 1:  k = ((ci / k_step)*ksize*ksize + ky*ksize + kx)*k_step + ci % k_step
 *               (channel-chunk-major: the 9 taps of one 64-channel slab are consecutive K steps, so the
 *                shifted re-reads of an input row hit L2 instead of the Infinity Cache)
 *   k_order 2:  direct small-channel kernel (Cin 16, 3x3): the weight stays in the reference layout
 *               [cout][cin][3][3] as f32 for either dtype; k_step = k_total = 144, cout_tile = cout.
 *               The kernel exists for PPN_F32 and PPN_BF16: ppn_conv2d_fused returns PPN_E_UNSUPPORTED for such a
 *               descriptor in PPN_F16 / PPN_F16X3 (those modes run the stem through ppn_stem012*)               */
int ppn_conv_tiling(int32_t dtype, int32_t cin, int32_t cout, int32_t ksize, int32_t* k_step, int32_t* cout_tile,
                    int32_t* k_order);

int ppn_conv2d_fused(const ppn_conv_desc* d, void* stream);

/* Workspace of a PPN_CONV_SPLIT_K launch of this descriptor (pointers are not looked at; the flag need not be set):
 * *bytes = slabs * batch * out_h * out_w * cout_pad * 4, *slabs = ceil(k_total / 512).  Returns what the launch would
 * return for a descriptor outside the split-K scope.  Host only. */
int ppn_conv_splitk_workspace(const ppn_conv_desc* d, int64_t* bytes, int32_t* slabs);

/* One launch per 64-channel stride-1 pre-activation BasicBlock (drn.py:25-57; DRN-D's layer3 behind its first block), 16-bit
 * modes (csrc/block64.hip, round 5):
 *   mid     = act_mid(conv3x3(src, weight1) * scale_mid + shift_mid)        never written to HBM
 *   v       = act1(conv3x3(mid, weight2) * scale1 + shift1) (+ residual)
 *   out_raw = v;   out_act = act2(v * scale2 + shift2)
 * i.e. the two ppn_conv2d_fused launches of the block (conv1 with out_raw = mid, conv2 reading it) in one persistent kernel:
 * `src` is the block's pre-activated input relu(bn1(x)), `residual` the raw x.  Both weights are packed [64][576] with
 * k = tap * 64 + ci (ppn_pack_weight k_order 0).  Outputs are BIT-IDENTICAL to the two launches (same K order, same epilogue
 * arithmetic, mid rounded to the 16-bit type as the stored tensor was).  All tensors NHWC [batch][h][w][64] of `dtype`. */
typedef struct ppn_block_desc {
    int32_t dtype;               /* PPN_BF16 or PPN_F16 */
    int32_t batch, h, w, channels;   /* channels = 64 */
    const void* src;
    const void* residual;        /* or NULL */
    const void* weight1;
    const float* scale_mid;      /* [64] or NULL (=1) */
    const float* shift_mid;      /* [64] or NULL (=0) */
    int32_t act_mid;
    const void* weight2;
    const float* scale1;
    const float* shift1;
    int32_t act1;
    const float* scale2;
    const float* shift2;
    int32_t act2;
    void* out_raw;               /* or NULL */
    void* out_act;               /* or NULL */
    int32_t flags;               /* 0 */
    /* stride 2 (round 5; 0 / 1 = the stride-1 block above): the FIRST block of layer3 (drn.py:168-190) -- conv1 is a 3x3
     * stride-2 convolution from 32 channels, `src` = relu(bn1(x)) NHWC [batch][in_h][in_w][32], weight1 packed [64][w1_ld] with
     * k = tap * 32 + ci (ppn_pack_weight k_order 0); the shortcut is bn_ds(conv1x1_stride2(x)): `proj_src` = x AT THE EVEN
     * PIXELS, NHWC [batch][h][w][32] (what the fused stem writes under PPN_STEM_RAW_S2), proj_weight packed [64][proj_ld] with
     * k = ci, proj_scale / proj_shift the folded BN; `residual` must be NULL.  Outputs [batch][h][w][64], h = (in_h - 1) / 2 + 1.
     * Bit-identical to the three ppn_conv2d_fused launches it replaces (downsample, conv1, conv2 + residual). */
    int32_t stride, in_h, in_w;
    const void* proj_src;
    const void* proj_weight;
    const float* proj_scale;
    const float* proj_shift;
    int32_t w1_ld, proj_ld;
} ppn_block_desc;
int ppn_basicblock64_fused(const ppn_block_desc* d, void* stream);

/* PPN_F16X3 helpers.
 * ppn_pack_weight_x3: w f32 [cout][cin][k][k] (device) -> out half [cout_pad][3 * k_pad], k_pad = k*k*cin (cin % 64 == 0),
 *   row layout per 64-channel slab sl: [half(ws) taps x 64 | half(ws - half(ws)) taps x 64 | half(ws * 2^-11) taps x 64]
 *   with ws = w * 2^scale_log2; the caller multiplies scale1 by 2^-scale_log2 (ppn_conv_desc.k_total = 3 * k_pad).
 * ppn_split_f16x3: src f32 NHWC [pixels][channels] -> dst half [pixels][hi(channels) | lo'(channels)]; channels % 8 == 0. */
int ppn_pack_weight_x3(const float* w, int32_t cout, int32_t cin, int32_t ksize, int32_t cout_pad, int32_t scale_log2,
                       void* out, void* stream);
int ppn_split_f16x3(const float* src, int64_t pixels, int32_t channels, void* dst, void* stream);

/* Where the launcher would cut the output pixels [0, m) of a conv with this Cin/Cout into two launches under tile
 * policy 2 (ppn_set_conv_tile_policy): *m_split pixels run whole rounds (256 CUs) of the most efficient large tile, the
 * remaining m - *m_split a smaller tile that fills one more round (e.g. 512 -> 512 at 32 x 48 x 48 = 73 728 pixels:
 * 65 536 on 256 x 256 tiles = 2 rounds, 8 192 on 128 x 128 tiles = 1 round, instead of 3 rounds of 192 x 256).
 * *m_split = 0: a single launch -- always under policies 0 and 1.  Each output element accumulates its GEMM depth in
 * the same order whatever tile computes it, so results do not depend on the cut. */
int ppn_conv_split(int32_t dtype, int32_t cin, int32_t cout, int64_t m, int64_t* m_split);

/*
 * Frame ingest (rt_test.py:150-157 grab_frame): cv2.resize(frame, (dst_w, dst_h)) [INTER_LINEAR, 8-bit fixed point],
 * cv2.flip(.,0) + cv2.flip(.,1) when `flip`, cv2.COLOR_BGR2RGB when `swap_rb`, on the device.
 *   src_bgr  u8 [batch, src_h, src_w, 3]   camera frames as cv2.VideoCapture.read() delivers them
 *   dst_rgb  u8 [batch, dst_h, dst_w, 3]   e.g. the conv plan's own input buffer (PoseProposalNet.input_buffer)
 * The arithmetic is OpenCV's (oracle/ingest_ref.py restates it; parity unpinned: cv2 is not in this image). */
int ppn_ingest_frames(const void* src_bgr, int32_t batch, int32_t src_h, int32_t src_w, void* dst_rgb, int32_t dst_h,
                      int32_t dst_w, int32_t flip, int32_t swap_rb, void* stream);

/*
 * Raw video frames (csrc/ingest.hip): what a hardware decoder (NV12, pitched), a raw ffmpeg pipe (I420) or a UVC camera
 * without conversion (YUYV) delivers, straight into dst u8 [batch][dst_h][dst_w][3] in ONE launch -- colour conversion,
 * resize, optional 180-degree flip and the store.  Every output byte equals converting the whole picture to RGB first and
 * then applying ppn_ingest_frames' resize rule (oracle/ingest_ref.py, incl. the exact-halving (a + b + c + d + 2) >> 2
 * path) and the flip; only the 4 taps an output pixel needs are converted, each saturated BEFORE the interpolation.
 *
 * Pixel rule: OpenCV's fixed-point cvtColor YUV -> RGB (modules/imgproc/src/color_yuv.simd.hpp; parity unpinned, as the
 * resize: cv2 is not in this image).  For a pixel's bytes Y, U, V and a set (CY, CVR, CVG, CUG, CUB, yoff), all int32:
 *     y = max(0, Y - yoff) * CY;  uu = U - 128;  vv = V - 128;  h = 1 << 19
 *     R = sat8((y + h + CVR * vv) >> 20)
 *     G = sat8((y + h + CVG * vv + CUG * uu) >> 20)
 *     B = sat8((y + h + CUB * uu) >> 20)
 * with an arithmetic shift and sat8 = clamp to 0..255; no term exceeds 6e8 in magnitude.  The sets are round(c * 2^20)
 * of the usual three-decimal constants (ppn_yuv_coefficients returns them; the first row is OpenCV's ITUR_BT_601_*):
 *     matrix, range            CY       CVR      CVG      CUG      CUB   yoff
 *     0 bt601, limited    1220542   1673527  -852492  -409993  2116026     16      (the default)
 *     1 bt709, limited    1220542   1880097  -558891  -223347  2214593     16
 *     0 bt601, full       1048576   1470104  -748826  -360853  1858077      0
 *     1 bt709, full       1048576   1651297  -490864  -196423  1945738      0
 * Chroma is the nearest sample, as in OpenCV: pixel (y, x) uses chroma sample (y >> 1, x >> 1) in NV12 and I420 and
 * (y, x >> 1) in YUYV.  Layouts:
 *     PPN_PIX_NV12  y: the Y plane [src_h][pitch];  u: interleaved U, V bytes [src_h / 2][pitch_c];  v: NULL
 *     PPN_PIX_I420  y: the Y plane;  u, v: [src_h / 2][pitch_c] planes of src_w / 2 bytes per row (YV12: swap u and v)
 *     PPN_PIX_YUYV  y: packed Y0 U Y1 V per pixel pair, [src_h][pitch];  u = v = NULL
 * Planes may have any alignment (the taps are byte loads).  dst is stored as dwords when dst_w % 4 == 0 and dst is 4-byte
 * aligned, as bytes otherwise (same bytes).  PPN_E_INVALID, before any launch: a NULL d, dst or required plane; an unknown
 * format or matrix; an odd src_w; an odd src_h in NV12 / I420; pitch or pitch_c below the row's bytes; frame_stride below
 * a plane's bytes ((rows - 1) * pitch + row bytes); a size below 1; batch or dst_h above 65535; src_h or src_w above 16384.
 * Runs on `stream`, allocates nothing, does not synchronise.
 */
#define PPN_PIX_NV12 0
#define PPN_PIX_I420 1
#define PPN_PIX_YUYV 2
typedef struct ppn_ingest_desc {
    int32_t format, batch, src_h, src_w;
    int32_t pitch;         /* bytes per row of the Y plane, or of the packed row for YUYV */
    int32_t pitch_c;       /* bytes per chroma row (NV12: >= src_w, I420: >= src_w/2; ignored for YUYV) */
    int64_t frame_stride;  /* bytes from one frame to the next, applied to each plane pointer */
    const void *y, *u, *v; /* NV12: u = the UV plane, v = NULL; YUYV: y = packed data, u = v = NULL */
    int32_t matrix;        /* 0 bt601, 1 bt709 */
    int32_t full_range;
    void* dst;
    int32_t dst_h, dst_w;
    int32_t flip;          /* both axes, as ppn_ingest_frames */
    int32_t dst_bgr;       /* 0: RGB */
} ppn_ingest_desc;
int ppn_ingest_yuv(const ppn_ingest_desc* d, void* stream);
int ppn_yuv_coefficients(int32_t matrix, int32_t full_range, int32_t out6[6]);   /* host only: the table above */

/*
 * Windowed inference (no counterpart in the reference, which squeezes every frame to the network's square input): a big
 * frame is cut into up to PPN_MAX_WINDOWS overlapping windows, every window runs as one image of the batch, and the people
 * of the windows are joined in frame pixels.  ONE layout serves every frame of a call (a fixed camera).  It is a host struct,
 * validated on the host and handed to the kernels by value: no device table, no synchronisation.  Image f * n + i of the
 * batch is window i of frame f.  A layout is bad (PPN_E_INVALID) when it is NULL, n is outside 1..PPN_MAX_WINDOWS, or a
 * window has h < 1, w < 1, y0 < 0 or x0 < 0.  tests/windows_ref.py restates both entry points in NumPy; kernels and
 * restatement agree on bytes.
 */
#define PPN_MAX_WINDOWS 16
typedef struct ppn_window { int32_t y0, x0, h, w; } ppn_window;      /* source pixels */
typedef struct ppn_window_layout { int32_t n; ppn_window win[PPN_MAX_WINDOWS]; } ppn_window_layout;

/*
 * ppn_ingest_windows (csrc/ingest.hip): the windows of F = d->batch raw frames into d->dst u8 [F * n][dst_h][dst_w][3], one
 * launch.  NORMATIVE: every output byte equals what ppn_ingest_yuv writes for a picture that consists of the window alone --
 * its planes cropped at (y0, x0) to h x w.  That covers the clamping of the taps at the WINDOW's borders (not the frame's),
 * the exact-halving path chosen per window (h == 2 * dst_h && w == 2 * dst_w) beside bilinear windows of the same launch,
 * the flip, dst_bgr and both store paths.  The per-axis scale is the host-computed double (double)w / (double)dst_w of the
 * window (h / dst_h).
 *
 * A fourth pixel format, accepted by this entry only (ppn_ingest_yuv refuses it): PPN_PIX_BGR24, packed B, G, R u8 per
 * pixel, y: [src_h][pitch] with pitch >= 3 * src_w, as cv2.VideoCapture delivers it; u, v, matrix and full_range are not
 * read (matrix must still be 0 or 1).  The rule is ppn_ingest_frames on the cropped picture with swap_rb = !dst_bgr: a
 * tap is the pixel's three bytes, there is no conversion.
 *
 * PPN_E_INVALID, before any launch: everything ppn_ingest_yuv refuses (for PPN_PIX_BGR24 the size may be odd); a bad
 * layout; a window that is not inside the picture; an odd x0 or w in a YUV format; an odd y0 or h in NV12 / I420;
 * F * n above 65535.  Runs on `stream`, allocates nothing, does not synchronise.
 */
#define PPN_PIX_BGR24 3
int ppn_ingest_windows(const ppn_ingest_desc* d, const ppn_window_layout* lay, void* stream);

/*
 * ppn_merge_windows (csrc/windows.hip): the people of the F * n window images (a ppn_decode result whose boxes are network
 * pixels of each image, inH x inW) -> per frame one people list in frame pixels, without the duplicates that overlapping
 * windows produce.  Every f32 step below is one IEEE operation rounded on its own (no contraction, IEEE division).
 *
 *   1 candidates   of frame f: for i = 0 .. n-1 and p = 0 .. min(max(count[f*n+i], 0), max_humans) - 1 the people with
 *                  kp_cell[f*n+i][p][0] >= 0 and a root score score[f*n+i][p][0] that is not NaN, in (i, p) order.  The
 *                  first PPN_MERGE_MAX_CAND take part; more set PPN_MERGE_FLAG_CAND_OVERFLOW.
 *   2 mapping      of window i: sy = (float)h / (float)inH, sx = (float)w / (float)inW; Y = y * sy + (float)y0 and
 *                  X = x * sx + (float)x0 (a multiply, then an add) on all four numbers (ymin, xmin, ymax, xmax) of every
 *                  present keypoint box.
 *   3 order        descending root score, compared as f32 values (-0.0 == +0.0); equal scores by ascending (i, p).
 *   4 greedy walk  in that order: candidate c is a DUPLICATE of the first kept candidate k before it with
 *                  window(k) != window(c) and iou(root_k, root_c) >= merge_thr on the mapped root boxes; without such a k,
 *                  c is KEPT.  iou is ppn_track_update's, operation for operation: areas a = (ymax - ymin) * (xmax - xmin),
 *                  tl = the larger ymin / xmin, br = the smaller ymax / xmax, inter = ((br0 - tl0) * (br1 - tl1)) *
 *                  [tl0 < br0 && tl1 < br1], iou = inter / ((a_k + a_c) - inter), a value that is not > 0 (a NaN included)
 *                  counts as 0.0f.  People of one window never suppress each other (the decode's own NMS has judged them);
 *                  duplicates suppress nobody.
 *   5 output order the kept candidates, in walk order, are output people 0, 1, ...; out_count[f] = their number; the first
 *                  max_out are written, more set PPN_MERGE_FLAG_OUT_OVERFLOW.
 *   6 keypoints    keypoint 0 is always the keeper's.  For j >= 1 with fuse != 0: among the keeper and its duplicates, in
 *                  walk order, that have keypoint j (kp_cell >= 0), the member with the largest score[j]; only a strictly
 *                  larger score (f32 comparison) replaces an earlier member.  With fuse == 0 only the keeper's own keypoints.
 *                  A written keypoint gets the member's mapped box, its score and out_src = i * max_humans + p of the
 *                  member (>= 0, so out_src serves as kp_cell for ppn_draw_humans and ppn_track_update); an absent keypoint
 *                  out_src = -1 and a zero box and score.  Rows at and above min(out_count[f], max_out) are not touched.
 *
 *   count i32 [F*n], kp_cell i32 [F*n][max_humans][K], bbox f32 [F*n][max_humans][K][4], score f32 [F*n][max_humans][K]
 *   out_count i32 [F], out_src i32 [F][max_out][K], out_bbox f32 [F][max_out][K][4] (ymin, xmin, ymax, xmax),
 *   out_score f32 [F][max_out][K], out_flags i32 [F] (written, not accumulated: the flags of this call)
 * One launch on `stream` (one workgroup per frame), no allocation, no host synchronisation, no atomics, integer and bitwise
 * reductions only: the call can be captured into a graph and two runs give identical bytes.  PPN_E_INVALID before anything
 * is launched for: a NULL pointer; K outside 1..PPN_MAX_KP; inH, inW or max_out < 1; max_humans outside 1..1024; frames < 1;
 * a bad layout; a merge_thr that is NaN; a bbox or out_bbox that is not 16-byte aligned.  Precondition: the boxes are finite;
 * otherwise which people are kept is unspecified, but no access leaves the buffers.
 */
#define PPN_MERGE_MAX_CAND 512
#define PPN_MERGE_FLAG_CAND_OVERFLOW 1
#define PPN_MERGE_FLAG_OUT_OVERFLOW 2
typedef struct ppn_merge_cfg {
    int32_t K, inH, inW, max_humans, max_out;
    float merge_thr;      /* default 0.3 = the decode's nms_thr */
    int32_t fuse;         /* 1: a kept person takes keypoints from its duplicates */
} ppn_merge_cfg;
int ppn_merge_windows(const ppn_merge_cfg* cfg, const ppn_window_layout* lay, const int32_t* count, const int32_t* kp_cell,
                      const float* bbox, const float* score, int32_t frames, int32_t* out_count, int32_t* out_src,
                      float* out_bbox, float* out_score, int32_t* out_flags, void* stream);

/*
 * Person crops (no counterpart in the reference, which stops at the drawn frame): every detected person of a frame cut out
 * of the RAW frame as a fixed-size picture for a following model.  Unlike a window layout the rectangles are DATA: a table
 * in device memory that ppn_people_rois writes from the people lists and ppn_ingest_rois reads, so that decode -> ROIs ->
 * crops is a chain of launches without a host synchronisation (it can be captured into a graph).  tests/crops_ref.py restates
 * both entries in NumPy; kernels and restatement agree on bytes.
 *
 * ppn_people_rois (csrc/crops.hip): a decode result (count, kp_cell, bbox as ppn_merge_windows takes them; the scores are
 * not read) -> roi i32 [F][max_rois][4] = (y0, x0, h, w) in source pixels and status i32 [F][max_rois].  Slot r of frame f
 * is PERSON r of that frame: no sorting, no top-k, the first max_rois people are taken, so a tracker's ids[f][r], bbox[f][r]
 * and crop r describe the same person.  The boxes are in pixels of some coordinate space (the network input for a plain
 * decode, the frame itself after ppn_merge_windows); the host passes sy = (float)src_h / (float)space_h and sx likewise.
 * Every f32 step below is one IEEE operation rounded on its own (no contraction, IEEE division).
 *
 *   1 person      slot r holds a person when r < min(max(count[f], 0), max_humans) and kp_cell[f][r][0] >= 0.  Otherwise
 *                 status = PPN_ROI_EMPTY and the ROI is (0, 0, 0, 0).
 *   2 box         mode PPN_ROI_MODE_ROOT: the root box bbox[f][r][0].  mode PPN_ROI_MODE_PEOPLE: the union of the boxes of
 *                 all present keypoints (kp_cell[f][r][j] >= 0), the smaller ymin / xmin and the larger ymax / xmax in
 *                 ascending j.  A number of a box that is used which is not finite makes the slot DEGENERATE (rule 7).
 *   3 mapping     Y = y * sy, X = x * sx on the four numbers (ymin, xmin, ymax, xmax).
 *   4 centre      cy = (ymin + ymax) * 0.5f;  hh = (ymax - ymin) * 0.5f;  hh = hh + hh * margin (a multiply, then an add);
 *                 the same for x, giving cx and hw.
 *   5 aspect      when aspect > 0 (the host's float dst_w / dst_h): if hw < hh * aspect then hw = hh * aspect, otherwise
 *                 hh = hw / aspect.  aspect == 0: the box keeps its shape.
 *   6 edges       t = floorf(cy - hh), b = ceilf(cy + hh), l = floorf(cx - hw), r = ceilf(cx + hw).  If one of the four is
 *                 not finite: DEGENERATE.  Each is limited to the picture as a float, fminf(fmaxf(v, 0), (float)src_h) for
 *                 rows, src_w for columns, and converted to int.  y0 = t rounded down and y1 = b rounded up to a multiple
 *                 of align_y, x0 / x1 likewise with align_x; h = y1 - y0, w = x1 - x0.  The ROI is the INTERSECTION with
 *                 the picture: it is neither shifted nor padded, so at a border the crop loses the requested aspect and
 *                 margin (ppn_ingest_rois stretches what is there to the output size).
 *   7 degenerate  unless h >= min_size && w >= min_size: status = PPN_ROI_DEGENERATE and the ROI is (0, 0, 0, 0).  A box
 *                 wholly outside the picture, a box too small, an inverted box, a NaN or an infinity anywhere land here.
 *   8 otherwise   status = PPN_ROI_OK and the ROI is (y0, x0, h, w): inside the picture, aligned, at least min_size, and it
 *                 contains the mapped box's part of the picture.
 *
 * Every slot of roi and status is written, rows of other frames or beyond max_rois are not.  One launch on `stream`, no
 * allocation, no host synchronisation, no atomics: two runs give identical bytes.  PPN_E_INVALID before anything is launched
 * for: a NULL pointer; K outside 1..PPN_MAX_KP; max_humans outside 1..1024; max_rois, frames or min_size < 1; src_h or src_w
 * outside 1..16384; align_y / align_x not 1 or 2, or one that does not divide the picture's size; min_size below an
 * alignment; an unknown mode; sy or sx not finite or not > 0; a margin that is NaN, negative or infinite; an aspect that is
 * NaN, negative or infinite; a bbox or roi that is not 16-byte aligned.
 */
#define PPN_ROI_OK 0
#define PPN_ROI_EMPTY 1          /* no person in the slot / an all-zero rectangle */
#define PPN_ROI_DEGENERATE 2     /* a person whose rectangle is below min_size, outside the picture or not finite */
#define PPN_ROI_BAD 4            /* ppn_ingest_rois: a rectangle that must not be read */
#define PPN_ROI_MODE_ROOT 0
#define PPN_ROI_MODE_PEOPLE 1
typedef struct ppn_roi_cfg {
    int32_t K, max_humans, max_rois;
    int32_t src_h, src_w;          /* the picture the ROIs are cut from */
    float sy, sx;                  /* box pixels -> source pixels */
    int32_t mode;                  /* PPN_ROI_MODE_* */
    float margin;                  /* added to each half size, as a fraction of it; default 0.1 */
    float aspect;                  /* dst_w / dst_h, or 0: keep the box's shape */
    int32_t align_y, align_x;      /* 1 or 2: NV12 / I420 need 2, 2; YUYV 1, 2; packed BGR 1, 1 */
    int32_t min_size;
} ppn_roi_cfg;
int ppn_people_rois(const ppn_roi_cfg* cfg, const int32_t* count, const int32_t* kp_cell, const float* bbox, int32_t frames,
                    int32_t* roi, int32_t* status, void* stream);

/*
 * ppn_ingest_rois (csrc/ingest.hip): the ROIs of F = d->batch raw frames into d->dst u8 [F * max_rois][dst_h][dst_w][3], one
 * launch; `d` is read as ppn_ingest_windows reads it (all four formats), `roi` is a DEVICE table i32 [F][max_rois][4] of
 * (y0, x0, h, w) and image f * max_rois + r is ROI r of frame f.  NORMATIVE: for a good ROI every output byte equals what
 * ppn_ingest_windows writes for a layout of one window holding that rectangle -- the clamping of the taps at the ROI's
 * borders, the exact-halving path chosen per ROI (h == 2 * dst_h && w == 2 * dst_w) beside bilinear ROIs of the same launch,
 * the flip, dst_bgr and both store paths.  The per-axis scale is the double (double)w / (double)dst_w, divided on the device
 * (an IEEE division: the host's bits).
 *
 * The table is data the host never sees, so it is judged on the device, per workgroup and before any tap:
 *   (0, 0, 0, 0)   an empty slot: the image is all zero bytes and status |= PPN_ROI_EMPTY;
 *   a bad ROI      (a negative origin; h < 1 or w < 1; a rectangle that leaves the picture; an odd x0 or w in a YUV format; an
 *                  odd y0 or h in NV12 / I420): the image is all zero bytes and status |= PPN_ROI_BAD.
 * Neither reads the source at all.  `status` i32 [F][max_rois] may be NULL; otherwise the bits are OR-ed into what it holds
 * (the table ppn_people_rois wrote, or zeros), by one work item per image and without atomics.
 *
 * PPN_E_INVALID, before any launch: everything ppn_ingest_windows refuses of `d`; a NULL roi; max_rois < 1; F * max_rois
 * above 65535.  Runs on `stream`, allocates nothing, does not synchronise.
 */
int ppn_ingest_rois(const ppn_ingest_desc* d, const int32_t* roi, int32_t max_rois, int32_t* status, void* stream);

/*
 * Train-time augmentation on the device (aug.py:13-160: IAA + ToNormalizedTensor), csrc/augment.hip.  Coordinates are pixel
 * indices with pixel centres at integers.  Per image the HOST builds the forward map F (source point -> output point:
 * rotation + isotropic scale about ((w-1)/2, (h-1)/2), minus the crop's (left, top), centre-aligned resize
 * x' = (x + 0.5) * out_w / w' - 0.5) and F^-1 in float64 and rounds both to f32 [2][3] (row-major: x row, y row); the
 * kernels use nothing else (augment.sample_params / affine_matrices).  All arithmetic below is f32 / i32 in exactly the
 * written order (no contraction), so the outputs are bit-exact with tests/augment_ref.py.  Both run on `stream` and
 * allocate nothing.
 *
 * ppn_augment_images: ONE bilinear resampling pass through F^-1.
 *   src      u8 [batch][src_h][src_w][3] RGB device, pictures padded to a common size (top-left aligned)
 *   src_hw   i32 [batch][2] device: valid (h, w) of each picture, <= (src_h, src_w)
 *   inv      f32 [batch][2][3] device
 *   dst_u8   u8 [batch][out_h][out_w][3] or NULL;  dst_f32  f32 [batch][3][out_h][out_w] or NULL (at least one):
 *            (float(v) - mean_c) / std_c, mean (0.485, 0.456, 0.406), std (0.229, 0.224, 0.225), no /255 (aug.py:149-153)
 * Per output pixel (ox, oy): sx = (inv00 * ox + inv01 * oy) + inv02, sy likewise; ix = floorf(sx), fx = sx - ix,
 * a1 = (int)rintf(fx * 2048), a0 = 2048 - a1 (b0, b1 for y); the taps (ix, iy) .. (ix + 1, iy + 1), a tap outside
 * [0, w) x [0, h) of THAT picture's valid size contributing 0 (constant border; padding and neighbours are never read);
 * per channel t0 = p00 * a0 + p01 * a1, t1 = p10 * a0 + p11 * a1, v = (b0 * t0 + b1 * t1 + (1 << 21)) >> 22.
 * 16-byte plane stores when out_w % 4 == 0 and the outputs are 16 / 4-byte aligned, scalar stores otherwise (same bits).
 *
 * ppn_augment_people: the label rules of aug.py:26-133 on the packed arrays of ppn_encode_targets (same layouts; K = the
 * keypoint count of that layout, people rows of 5 + 2 * (K - 1) floats), one workgroup per image.
 *   keypoint (0, 0): absent, stays (0, 0).  Otherwise x' = (f00 * x + f01 * y) + f02, y' likewise; kept iff
 *   0 <= x' < out_w and 0 <= y' < out_h, else (0, 0).  A keypoint that is (0, 0) afterwards loses its visible bit; no bit is
 *   ever set; hidden keypoints that stay in frame keep their coordinates.
 *   head box (cx, cy, w, h): corners cx -+ floorf(w / 2), cy -+ floorf(h / 2), all four through F, min / max per axis,
 *   clipped to [0, out_w] x [0, out_h], stored as ((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1).  `size` is copied.
 *   A person whose 2 * (K - 1) keypoint values are all 0 is removed; the survivors keep their order (any pmax);
 *   count_out[b] = survivors (0 when nobody is left), rows beyond it are zeroed in people_out and visible_out.
 * The outputs must not alias the inputs.
 *
 * Options of the stage (not in aug.py; NumPy restatement tests/augment_jitter_ref.py).  With both off nothing above changes.
 *
 * Left-right mirror.  The HOST composes the reflection x -> (w - 1) - x (w = the picture's valid width) into F and F^-1,
 * applied to the source point before the rotation; the image kernels need nothing else.  The labels additionally swap
 * their left / right slots:
 * ppn_augment_people_mirror: every rule of ppn_augment_people, and in an image with mirror[b] != 0 output point slot j
 *   (keypoint j + 1; keypoint 0, the instance, has no slot) takes input point slot mj = kp_mirror[j + 1] - 1: its
 *   coordinates, which then go through F, and its visible bit (output bit j = input bit mj, cleared afterwards if the mapped
 *   point is (0, 0)).  Visible bits K - 1 and above have no slot and are copied.  The head box and `size` are not permuted.
 *   mirror     i32 [batch] device, or NULL: nobody is mirrored.  NULL or a flag of 0 gives ppn_augment_people's bytes.
 *   kp_mirror  i32 [K] HOST (tta.mirror_tables()): validated here, an involution on 0..K-1 with kp_mirror[0] == 0, and
 *              passed to the kernel by value.
 *   PPN_E_INVALID: a NULL pointer other than mirror, an output that is one of the inputs, K outside 1..PPN_MAX_KP, a
 *   non-positive size, a table that is not such an involution; nothing is launched then.
 *
 * Colour and noise.
 * ppn_augment_images_color: ppn_augment_images with a colour step between the interpolation and the stores.
 *   color  i32 [batch][10] device: {sat, gain_r, gain_g, gain_b, off_r, off_g, off_b, noise_q, key_lo, key_hi}; the kernel
 *          clamps sat to 0..512, gain to 0..1024, off to -255..255 and noise_q to 0..4096 (256 = factor 1).
 *   (r, g, b) = the three interpolated v of the pixel.  All arithmetic is i32; `>>` on a negative value is an arithmetic
 *   (floor) shift.
 *     1. y = (77 r + 150 g + 29 b + 128) >> 8;  per channel c1 = clamp(y + (((c - y) * sat + 128) >> 8), 0, 255)
 *     2. c2 = ((c1 * gain_c + 128) >> 8) + off_c
 *     3. idx = oy * out_w + ox;  z = output number idx (0-based) of the splitmix64 stream started at
 *        key = (u32)key_lo | (u64)(u32)key_hi << 32, i.e. prng.raw_u64(key, out_h * out_w)[idx]: z = key + (idx + 1) *
 *        0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31
 *        (u64, wrap-around).  Channel c = 0, 1, 2 (r, g, b): t = (z >> 21 c) & 0x1FFFFF,
 *        s = 2 * ((t & 127) + ((t >> 7) & 127) + ((t >> 14) & 127)) - 381,  d = (s * noise_q + (1 << 13)) >> 14
 *        (zero mean, sd = noise_q / 128 in u8 units; the same key gives every image the same field).
 *     4. c3 = clamp(c2 + d, 0, 255)
 *   dst_u8 receives c3, dst_f32 ((float)c3 - mean_c) / std_c.  The step applies to EVERY output pixel, the constant-0 border
 *   included (a partly covered pixel cannot be told from it).  The row (256, 256, 256, 256, 0, 0, 0, 0, *, *) reproduces
 *   ppn_augment_images bit for bit.  PPN_E_INVALID as ppn_augment_images, and for a NULL color or an output that is one of
 *   the inputs.
 */
int ppn_augment_images(const uint8_t* src, const int32_t* src_hw, const float* inv, int32_t batch, int32_t src_h,
                       int32_t src_w, int32_t out_h, int32_t out_w, uint8_t* dst_u8, float* dst_f32, void* stream);
int ppn_augment_people(const float* people, const int32_t* visible, const int32_t* count, const float* fwd, int32_t batch,
                       int32_t pmax, int32_t K, int32_t out_h, int32_t out_w, float* people_out, int32_t* visible_out,
                       int32_t* count_out, void* stream);
int ppn_augment_images_color(const uint8_t* src, const int32_t* src_hw, const float* inv, const int32_t* color, int32_t batch,
                             int32_t src_h, int32_t src_w, int32_t out_h, int32_t out_w, uint8_t* dst_u8, float* dst_f32,
                             void* stream);
int ppn_augment_people_mirror(const float* people, const int32_t* visible, const int32_t* count, const float* fwd,
                              const int32_t* mirror, const int32_t* kp_mirror, int32_t batch, int32_t pmax, int32_t K,
                              int32_t out_h, int32_t out_w, float* people_out, int32_t* visible_out, int32_t* count_out,
                              void* stream);

/*
 * Drawing the decoded people on the device (datatest.py:162-232, draw_humans), csrc/render.hip: a tiled rasteriser over
 * the compact decode result that paints exactly the pixels PIL's ImageDraw paints for the reference's calls (established
 * against Pillow 12.2; tests/render_ref.py restates the rules below in NumPy, tests/golden/draw_cases.npz holds frames the
 * reference itself drew).  All f32 arithmetic is in the written order, uncontracted, with IEEE division.
 *
 * Paint order: people 0 .. min(count, max_humans) - 1 in order; within a person the keypoints kp_order[0 .. K-1] that are
 * present (kp_cell >= 0), then the limbs e = 0 .. E-1 whose two ends are present; a later primitive overwrites an earlier
 * one.  T(v) is truncation toward zero of an f32, midpoints are (a + b) / 2 in f32, a box is (ymin, xmin, ymax, xmax).
 *   root (keypoint 0)   two one-pixel rectangle outlines in palette[0]: [T(xmin), T(ymin), T(xmax), T(ymax)] and the same
 *                       box shrunk by 1 on every side.  An outline [x0, y0, x1, y1] is the border of that pixel box; with
 *                       x1 < x0 or y1 < y0 it draws nothing.
 *   keypoint k > 0      visbbox: one such outline of its box in palette[k].  Otherwise a disc: with (x, y) the box centre,
 *                       bx0 = T(x - 2), by0 = T(y - 2), bx1 = T(x + 2), by1 = T(y + 2); the pixel box [bx0, by0, bx1, by1]
 *                       (4 or 5 pixels each way) without its four corner pixels.
 *   limb (s, t)         PIL's width-2 line from (x0, y0) to (x1, y1), the truncated box centres of s and t, in palette[s].
 *                       dx = x1 - x0, dy = y1 - y0; a zero vector draws the pixel (x0, y0).  Otherwise
 *                       dxmax = RD(dy / hypot(dx, dy)), dymax = RU(dx / hypot(dx, dy)) with
 *                       RU(f) = floor(f + .5) for f >= 0, -floor(|f| + .5) otherwise, RD(f) = ceil(f - .5) for f >= 0,
 *                       -ceil(|f| - .5) otherwise (so dxmax = sign(dy) iff 3 dy^2 > dx^2, dymax = sign(dx) iff
 *                       3 dx^2 > dy^2, else 0), and the quad (x0, y0 + dymax), (x1, y1 + dymax), (x1 + dxmax, y1),
 *                       (x0 + dxmax, y0) is filled by scan lines over its four edges (vertex i to vertex i + 1):
 *                       a horizontal edge is drawn as its own clipped horizontal line.  ymin = min(H - 1, the edges'
 *                       smallest y), ymax = max(0, their largest y), then ymin = max(ymin, 0), ymax = min(ymax, H).  For
 *                       each row y in [ymin, ymax]: over the non-horizontal edges e (from (ex0, ey0), f32 slope
 *                       s = (float)(ex1 - ex0) / (float)(ey1 - ey0)) whose y range holds y, collect
 *                       x = (float)(y - ey0) * s + (float)ex0, twice when y is the edge's largest y and y < ymax; sort;
 *                       fill [RU(x[i-1]), RD(x[i])] for i = 1, 3, .., a reversed pair swapped, clipped to the frame.
 *                       The rule is not symmetric in the end points and, rounding being symmetric about zero, not
 *                       translation-invariant: it is evaluated in frame coordinates.
 *   grid                after all people, every column x = 0, grid_step, .. < W and every row y = 0, grid_step, .. < H in
 *                       (110, 110, 110).
 * A keypoint any of whose four box values is not finite or has |v| >= 2^20 is treated as absent (its limbs too).
 * Deviations from the reference: PIL raises for an outline with x1 < x0 or y1 < y0 (here: nothing is drawn), paints two
 * stray pixels below an outline of zero height (here: none), and raises or takes seconds on the out-of-range coordinates;
 * the mask= paste is not built.
 *
 *   src, dst   u8 [batch][height][width][3] RGB device.  dst == src draws in place and stores only drawn pixels; otherwise the
 *              two must not overlap and every pixel of dst is written (12-byte stores when width % 4 == 0 and both are
 *              4-byte aligned)
 *   count      i32 [batch], kp_cell i32 [batch][max_humans][K], bbox f32 [batch][max_humans][K][4]: ppn_decode's outputs
 *   workspace  ppn_draw_workspace_bytes(cfg, batch, max_humans) bytes, 16-byte aligned: 48 bytes per (person, slot)
 * Two launches on `stream`, no allocation, no host synchronisation.  Limits (PPN_E_UNSUPPORTED beyond them): batch <= 65535,
 * height and width <= 32768, max_humans * (K + E) < 2^30.  Any number of primitives may cover one tile.
 */
typedef struct ppn_draw_cfg {
    int32_t K, E;
    int32_t edge_src[PPN_MAX_EDGES], edge_dst[PPN_MAX_EDGES]; /* limbs in EDGES order */
    int32_t kp_order[PPN_MAX_KP];                             /* paint order of the keypoints: K entries in [0, K) */
    uint8_t palette[PPN_MAX_KP][4];                           /* r, g, b, unused */
    int32_t visbbox, grid, grid_step;                         /* grid_step >= 1 when grid is set */
} ppn_draw_cfg;

size_t ppn_draw_workspace_bytes(const ppn_draw_cfg* cfg, int32_t batch, int32_t max_humans); /* 0 on a bad argument */
int ppn_draw_humans(const ppn_draw_cfg* cfg, const uint8_t* src, uint8_t* dst, int32_t batch, int32_t height, int32_t width,
                    const int32_t* count, const int32_t* kp_cell, const float* bbox, int32_t max_humans, void* workspace,
                    void* stream);

/*
 * Drawing onto raw video surfaces (csrc/render.hip): the people painted straight onto NV12, I420 or YUYV frames -- what
 * ppn_ingest_yuv reads -- in place or into a second surface, in one pass, without an RGB intermediate; the result is what
 * an encoder or a raw pipe takes.  tests/render_yuv_ref.py restates both rules below in NumPy; kernel and restatement
 * agree on every byte.
 *
 * Forward colour rule (NORMATIVE).  For a colour (R, G, B) and a set (matrix, range), all int32, arithmetic shift,
 * sat8 = clamp to 0..255:
 *     Y = sat8((CYR * R + CYG * G + CYB * B + (1 << 19) + (yoff << 20)) >> 20)
 *     U = sat8((CUR * R + CUG * G + CUB * B + (1 << 19) + (128 << 20)) >> 20)
 *     V = sat8((CVR * R + CVG * G + CVB * B + (1 << 19) + (128 << 20)) >> 20)
 * The coefficients are round(c * 2^20) of the exact definitions Y' = Kr R + (1 - Kr - Kb) G + Kb B, U = (B - Y') / (2 (1 - Kb)),
 * V = (R - Y') / (2 (1 - Kr)) with BT.601's Kr 0.299, Kb 0.114 and BT.709's Kr 0.2126, Kb 0.0722; limited range scales luma
 * by 219 / 255 and chroma by 224 / 255, full range by 1 with yoff 0.  The G coefficient of U and of V is minus the sum of the
 * other two, so every grey has U = V = 128 exactly.  No accumulator exceeds 2.7e8.
 *     matrix, range          CYR     CYG     CYB       CUR      CUG     CUB      CVR      CVG     CVB   yoff
 *     0 bt601, limited    269262  528618  102662   -155423  -305128  460551   460551  -385654  -74897     16   (the default)
 *     1 bt709, limited    191455  644067   65019   -105533  -355018  460551   460551  -418321  -42230     16
 *     0 bt601, full       313524  615514  119538   -176932  -347356  524288   524288  -439026  -85262      0
 *     1 bt709, full       222927  749942   75707   -120138  -404150  524288   524288  -476214  -48074      0
 * Full range reaches 256 before sat8 (pure blue's U, pure red's V); limited range stays within 16..235 (Y) and 16..240 (U, V).
 * This is the project's own rule: it is NOT OpenCV's RGB -> YUV table (three-decimal constants) and NOT the algebraic inverse
 * of ppn_ingest_yuv's rule, whose sets come from other constants -- a drawn colour read back through the ingest differs from
 * the palette's by a few levels (profiles/render_yuv.txt).  ppn_rgb_to_yuv applies it on the host to n packed triples
 * (rgb and yuv may be the same buffer); it needs no GPU.
 *
 * Paint rule (NORMATIVE).  Let P(y, x) be what ppn_draw_humans decides for a height x width frame: unpainted, or the RGB
 * colour of the last covering primitive, the grid on top when enabled.  The palette and the grid's grey are converted once,
 * on the host; the kernel does no colour arithmetic.
 *   luma     sample (y, x) becomes Y(P(y, x)) where the pixel is painted and keeps the source byte otherwise.
 *   chroma   a sample belongs to a group of pixels: the 2 x 2 block (2i .. 2i + 1, 2j .. 2j + 1) in NV12 / I420, the pair
 *            (y, 2j .. 2j + 1) in YUYV.  With no painted pixel in the group it keeps the source bytes; otherwise U and V are
 *            those of the colour of the FIRST painted pixel of the group in row-major order (the final colours: after all
 *            people and the grid).  Not the top-left pixel alone, as OpenCV samples RGB -> YUV420: limbs are 2 pixels wide
 *            and outlines 1, so an outline on an odd row or column would keep the background's chroma.
 *   dst == src in every plane and in pitch, pitch_c and frame_stride: in place; only painted luma samples and the chroma
 *            samples of groups with a painted pixel are stored.  Otherwise out of place: no dst plane may be a src plane (nor
 *            overlap one), every content byte of every dst plane is written and the bytes between a row's content and its
 *            pitch never are.  Unpainted samples are copied, never converted: repeated annotation does not degrade a picture.
 * Planes are laid out as ppn_ingest_desc's (NV12: u = the interleaved UV plane, v = NULL; I420: YV12 swaps u and v; YUYV:
 * y = the packed rows, u = v = NULL) and may have any alignment and pitch: out of place the kernel stores dwords (halfwords
 * in I420's chroma planes) when width % 4 == 0 and every plane, pitch and frame_stride of both surfaces is a multiple of
 * 4 (2 for I420's chroma), bytes otherwise -- the same bytes.
 *
 * PPN_E_INVALID, before any launch: everything ppn_draw_humans refuses (height and width are the surface's); a NULL surface
 * or required plane; an unknown format (PPN_PIX_BGR24 included) or matrix; an odd width; an odd height in NV12 / I420; pitch or
 * pitch_c below the row's bytes; frame_stride below a plane's bytes ((rows - 1) * pitch + row bytes); src and dst that differ
 * in format, size, matrix or range; a dst plane equal to its src plane while another plane, a pitch or the stride differs.
 * The size limits are ppn_draw_humans' (PPN_E_UNSUPPORTED).  workspace: ppn_draw_workspace_bytes.  Two launches on `stream`,
 * no allocation, no host synchronisation.
 */
typedef struct ppn_yuv_surface {
    int32_t format;        /* PPN_PIX_NV12, PPN_PIX_I420 or PPN_PIX_YUYV */
    int32_t height, width;
    int32_t pitch;         /* bytes per row of the Y plane, or of the packed row for YUYV */
    int32_t pitch_c;       /* bytes per chroma row (NV12: >= width, I420: >= width / 2; ignored for YUYV) */
    int64_t frame_stride;  /* bytes from one frame to the next, applied to each plane pointer */
    void *y, *u, *v;
    int32_t matrix;        /* 0 bt601, 1 bt709 */
    int32_t full_range;
} ppn_yuv_surface;
int ppn_rgb_to_yuv(int32_t matrix, int32_t full_range, const uint8_t* rgb, uint8_t* yuv, int64_t n);   /* host only */
int ppn_draw_humans_yuv(const ppn_draw_cfg* cfg, const ppn_yuv_surface* src, const ppn_yuv_surface* dst, int32_t batch,
                        const int32_t* count, const int32_t* kp_cell, const float* bbox, int32_t max_humans, void* workspace,
                        void* stream);

/*
 * Redaction (no counterpart in the reference; csrc/redact.hip): the detected people -- by default their heads -- made
 * unrecognisable in the RAW frame before it leaves the box, in the format the encoder takes, without an RGB round trip and
 * without a host synchronisation.  Two launches: ppn_redact_cells turns people lists and a small hold state into per-frame
 * bit masks over a grid of square cells, ppn_redact_yuv applies a mask to raw surfaces.  tests/redact_ref.py restates both
 * in NumPy; kernels and restatement agree on every byte.  Not built: blur, ellipses, a per-track hold that follows a moving
 * person, MultiLaneInference integration.  No claim is made about how well the neck + top boxes cover a face: the
 * synthetic checkpoints say nothing about that.
 *
 * The cell grid.  Cells are cell x cell luma pixels, cell in {8, 16, 32}.  A src_h x src_w picture has CH = ceil(src_h / cell)
 * rows and CW = ceil(src_w / cell) columns of cells; those of the last row or column may be partial.  A frame's mask is
 * u32 [CH][MW], MW = ceil(CW / 32): cell (cy, cx) is bit cx & 31 of word [cy][cx >> 5].  A reader ignores the bits at and
 * above CW of a row's last word.  cell is even, so a cell's pixels own whole chroma groups in every format.
 *
 * ppn_redact_cells: a decode result (count, kp_cell, bbox as ppn_people_rois takes them) -> mask and flags.  Image
 * b = s * frames + t is frame t of stream s (the tracker's layout); streams are independent, the frames of a stream are
 * taken in ascending t within a call and from call to call.  Every f32 step is one IEEE operation rounded on its own.
 *
 * Person p of image b takes part when p < min(max(count[b], 0), max_humans) and kp_cell[b][p][0] >= 0.  Then:
 *   1 set      the keypoints j < K with bit j of kp_mask set and kp_cell[b][p][j] >= 0.  If there are none:
 *              PPN_REDACT_FALLBACK_PERSON takes all present keypoints j < K (the root is one, so the set is not empty:
 *              better to hide too much than to show a face); PPN_REDACT_FALLBACK_NONE: the person contributes nothing.
 *   2 box      the union of the set's boxes in ascending j: the first box, then per further box the smaller ymin / xmin
 *              (v < b ? v : b) and the larger ymax / xmax (v > b ? v : b).  If a number of a box of the set is not finite,
 *              the person contributes nothing and PPN_REDACT_FLAG_BAD_BOX is set.  Boxes outside the set do not count, whatever
 *              they hold.
 *   3 mapping  ppn_people_rois' rules 3 and 4, operation for operation, without the aspect rule: Y = y * sy, X = x * sx;
 *              cy = (ymin + ymax) * 0.5f; hh = (ymax - ymin) * 0.5f; hh = hh + hh * margin; cx and hw likewise.
 *   4 edges    t = floorf(cy - hh), b = ceilf(cy + hh), l = floorf(cx - hw), r = ceilf(cx + hw).  If one of the four is
 *              not finite: nothing, and BAD_BOX.  Each is limited as a float, fminf(fmaxf(v, 0), (float)src_h) for rows,
 *              src_w for columns, and converted to int.  t >= b or l >= r: nothing (a box outside the picture or an
 *              inverted box is no error).
 *   5 cells    the person covers the cell rows t / cell .. (b - 1) / cell and columns l / cell .. (r - 1) / cell
 *              (integer divisions; both ends included).
 * covered(c) is the OR over the image's people.  flags[b] = PPN_REDACT_FLAG_BAD_BOX if any person of image b set it, else
 * 0: written, not accumulated.
 *
 * Hold.  ttl u8 [streams][CH][CW] holds one byte per cell and stream; all zero is a fresh state and zeroing it is the reset.
 * Per frame and cell: ttl' = covered ? hold + 1 : (ttl > 0 ? ttl - 1 : 0), and the cell's mask bit is ttl' > 0 -- a cell
 * stays masked for `hold` more frames after the last frame that covered it.  With hold == 0 the mask is `covered` and ttl
 * is neither read nor written (it may be NULL).  A cell's history depends on no other cell.
 *
 * Every word of mask [streams * frames][CH][MW] and of flags [streams * frames] is written, bits at and above CW as 0;
 * with hold > 0 every byte of ttl is.  One launch on `stream`, no atomics, no allocation, no host synchronisation: the call
 * can be captured into a graph and two runs from the same state give identical bytes.  PPN_E_INVALID before any launch
 * for: a NULL pointer (ttl may be NULL iff hold == 0); K outside 1..PPN_MAX_KP; max_humans outside 1..1024; streams or
 * frames < 1 (or streams above 65535); src_h or src_w outside 1..16384; cell not 8, 16 or 32; sy or sx not finite or not
 * > 0; a margin that is NaN, negative or infinite; hold outside 0..254; an unknown fallback; a kp_mask without a bit below
 * K; a bbox that is not 16-byte aligned.
 */
#define PPN_REDACT_FALLBACK_PERSON 0
#define PPN_REDACT_FALLBACK_NONE 1
#define PPN_REDACT_FLAG_BAD_BOX 1
typedef struct ppn_redact_cells_cfg {
    int32_t K, max_humans;
    int32_t src_h, src_w, cell;
    float sy, sx;            /* box pixels -> source pixels, as ppn_roi_cfg */
    uint32_t kp_mask;        /* bit j: keypoint j belongs to the region (default: neck | top = the head) */
    int32_t fallback;        /* PPN_REDACT_FALLBACK_PERSON (default) | PPN_REDACT_FALLBACK_NONE */
    float margin;            /* as ppn_roi_cfg.margin; default 0.25 */
    int32_t hold;            /* 0..254 frames a cell stays masked after it was last covered */
} ppn_redact_cells_cfg;
int ppn_redact_cells(const ppn_redact_cells_cfg* cfg, uint8_t* ttl, const int32_t* count, const int32_t* kp_cell,
                     const float* bbox, int32_t streams, int32_t frames, uint32_t* mask, int32_t* flags, void* stream);

/*
 * ppn_redact_yuv: masks u32 [batch][CH][MW] (device; CH, CW, MW from the surface's height and width and cfg->cell) ->
 * redacted surfaces.  The surfaces are ppn_draw_humans_yuv's (NV12, I420, YUYV: any pitch and alignment, frame_stride);
 * this entry also takes PPN_PIX_BGR24 as ppn_ingest_windows does: y = the packed B, G, R bytes, pitch >= 3 * width, the
 * size may be odd, u, v, pitch_c, matrix and full_range are not read.
 *
 * A masked cell (cy, cx) owns these sample sets, every one clipped to the picture:
 *   luma              the pixels (y, x), y in [cy * cell, min((cy + 1) * cell, height)), x likewise with width
 *   NV12 / I420       U and V each on their own: the chroma samples (i, j), i in [cy * cell / 2, min((cy + 1) * cell / 2,
 *                     height / 2)), j in [cx * cell / 2, min((cx + 1) * cell / 2, width / 2))
 *   YUYV              U and V each on their own: rows as luma, j in [cx * cell / 2, min((cx + 1) * cell / 2, width / 2))
 *   BGR24             the three channels each on their own, over the luma set
 * PPN_REDACT_MOSAIC: every sample of a set becomes the set's rounded mean (s + (n >> 1)) / n, s the sum and n the number
 * of the set's samples INSIDE the picture (not cell * cell at a border), an integer division.  The sums stay below
 * 1024 * 255, and integer sums give the same bytes in any order.  The mean of equal values is that value: redacting a
 * redacted frame again with the same mask changes nothing.  PPN_REDACT_FILL: every sample of a set takes its plane's byte
 * of cfg->fill: fill[0] luma, fill[1] U, fill[2] V (ppn_rgb_to_yuv converts a colour); BGR24: fill[0..2] in memory order.
 * Samples of unmasked cells keep their bytes.  Mask bits at and above CW are ignored.
 *
 * dst == src in every plane and in pitch, pitch_c and frame_stride: in place; only samples of masked cells are stored, and
 * a cell is read completely before any of it is written, by the one wave that owns it.  Otherwise out of place: no dst
 * plane may be a src plane (nor overlap one), every content byte of every dst plane is written (unmasked samples are
 * copied) and the bytes between a row's content and its pitch never are.  The kernel moves dwords (a row's
 * last 1..3 bytes of a cell at the picture's border as bytes) when every plane pointer, pitch, pitch_c and frame_stride of
 * both surfaces is a multiple of 4, bytes otherwise -- the same bytes.
 *
 * One launch on `stream`, no allocation, no host synchronisation, no atomics.  PPN_E_INVALID before any launch: everything
 * ppn_draw_humans_yuv refuses of a surface pair, except that PPN_PIX_BGR24 is accepted (a NULL surface or required plane,
 * an unknown format, an unknown matrix of a YUV surface, an odd width or an odd NV12 / I420 height, a pitch or frame_stride
 * below the content, surfaces that differ in format or size -- for YUV also in matrix or range --, a shared plane without
 * everything shared); a NULL cfg or mask; cell not 8, 16 or 32; an unknown mode; batch < 1 or above 65535; height or width
 * above 16384.
 */
#define PPN_REDACT_MOSAIC 0
#define PPN_REDACT_FILL 1
typedef struct ppn_redact_cfg {
    int32_t cell;            /* 8, 16, 32: the mask's grid */
    int32_t mode;            /* PPN_REDACT_MOSAIC | PPN_REDACT_FILL */
    uint8_t fill[4];         /* FILL: Y, U, V (BGR24: the three bytes in memory order), unused */
} ppn_redact_cfg;
int ppn_redact_yuv(const ppn_redact_cfg* cfg, const ppn_yuv_surface* src, const ppn_yuv_surface* dst, int32_t batch,
                   const uint32_t* mask, void* stream);

/*
 * The per-image matching of a validation epoch on the device (main.py:1017-1172 validate / 886-1014 test_output ->
 * datatest.evaluation -> eval_helpers.assignGTmulti, eval_helpers.py:300-468), csrc/validate.hip: one batch of compact
 * people lists against the resident ground truth of the whole validation set, one workgroup per image, emitting the
 * per-person, per-joint (score, label) records evaluate.assign_gt_multi produces (tests/validate_ref.py restates the rules
 * below in NumPy; tests/golden/eval_cases.npz pins them to the reference).  K = 18: keypoint 0 is the instance, keypoint
 * j + 1 is joint j of the PPN_MATCH_JOINTS = 17.
 *
 * For batch image b with n = image_index[b], P = min(max(count[b], 0), max_humans), G = gt_count[n]:
 *   predicted joint j   of person p is present iff kp_cell[b][p][j + 1] >= 0; its point is x = (box[1] + box[3]) / 2,
 *                       y = (box[0] + box[2]) / 2 of its box (ymin, xmin, ymax, xmax), its score score[b][p][j + 1].  A missing
 *                       joint is the point (0, 0) with score 0 and takes part in the matching like any other.
 *   match[p][g][j]      sqrt(dx * dx + dy * dy) / gt_head[n][g] <= dist_thresh with dx = gt_x - x, dy = gt_y - y: every step
 *                       an f32 operation rounded on its own (no contraction, IEEE square root and division, no reciprocal),
 *                       the comparison in f32.  A NaN or infinite quotient (head size 0) is no match.
 *   cnt[p][g]           the number of matching joints; comparisons are on these integers.
 *   best_gt[p]          the first g with the largest cnt[p][.].
 *   claim               ground-truth person g is claimed by the first p, in ascending p, with the largest cnt[p][g] among the
 *                       p whose best_gt is g; a largest value of 0 claims nobody.
 *   rec_label[n][p][j]  match[p][g][j] for the one g that p claimed, otherwise 0;  rec_score[n][p][j] the joint's score.
 *   rec_count[n]        P when G > 0, otherwise 0: a frame without ground truth is dropped with its predictions (cleanupData).
 * Rows p < rec_count[n] of rec_score / rec_label are written and no others; rec_count[n] is written whenever n is valid.
 * image_index[b] == -1 marks a padding image of a ragged last batch: nothing is written for it.  The valid indices of one
 * call must differ from each other.  Errors found on the device OR a bit into *flags (which the caller zeroes once per epoch)
 * and write nothing for that image: PPN_MATCH_FLAG_INDEX for an index outside [-1, n_images), PPN_MATCH_FLAG_GT_COUNT for a
 * gt_count outside [0, gmax].
 *
 *   count       i32 [batch], kp_cell i32 [batch][max_humans][18], bbox f32 [batch][max_humans][18][4] (16-byte aligned),
 *               score f32 [batch][max_humans][18]: ppn_decode's outputs as they live on the device
 *   gt_xy       f32 [n_images][gmax][17][2] (x, y; 8-byte aligned), gt_head f32 [n_images][gmax], gt_count i32 [n_images]
 *   rec_score   f32 [n_images][max_humans][17], rec_label u8 [n_images][max_humans][17], rec_count i32 [n_images]: buffers
 *               of a whole epoch, rows addressed by image_index, so that an epoch needs one D2H at its end
 * One launch on `stream`, no allocation, no host synchronisation, no D2H: the call can be captured into a graph.  Integer
 * maxima only, no floating-point atomics: two runs give identical bytes.  Limits (PPN_E_UNSUPPORTED beyond them):
 * gmax <= PPN_MATCH_MAX_GT, max_humans <= PPN_MATCH_MAX_PEOPLE.
 */
#define PPN_MATCH_JOINTS 17
#define PPN_MATCH_MAX_GT 64
#define PPN_MATCH_MAX_PEOPLE 1024
#define PPN_MATCH_FLAG_INDEX 1
#define PPN_MATCH_FLAG_GT_COUNT 2

int ppn_pckh_match(const int32_t* count, const int32_t* kp_cell, const float* bbox, const float* score, int32_t batch,
                   int32_t max_humans, const float* gt_xy, const float* gt_head, const int32_t* gt_count, int32_t n_images,
                   int32_t gmax, const int32_t* image_index, float dist_thresh, float* rec_score, uint8_t* rec_label,
                   int32_t* rec_count, int32_t* flags, void* stream);

/*
 * Tracking people across the frames of a video on the device (no counterpart in the reference, whose rt_test.py treats every
 * frame on its own), csrc/track.hip: the compact people lists of B = streams * frames images against up to PPN_TRACK_SLOTS
 * resident tracks per stream, giving every person a track id that follows the human from frame to frame, and its keypoint
 * centres smoothed over time.  tests/track_ref.py restates the rules below in NumPy; kernel and restatement agree on bytes.
 *
 * Batch layout: image b = s * frames + t is frame t of stream s.  The streams of a call are independent; the frames of a
 * stream are processed in ascending t within the one call.  With n_frames given only t < n_frames[s] are processed (a
 * negative n_frames[s] counts as 0); for every other image all out_id entries are -1, all out_hits entries 0, out_live is -1,
 * out_xy is not written, and a stream without a processed frame leaves its state and its flags word untouched.
 *
 * Per processed image: P = min(max(count[b], 0), max_humans) and D = min(P, PPN_TRACK_MAX_DET); P > D sets
 * PPN_TRACK_FLAG_DET_OVERFLOW and people p >= D take no part, nor does a person whose kp_cell[b][p][0] < 0.  Keypoint k of a
 * person is present iff kp_cell[b][p][k] >= 0; its centre is x = (box[1] + box[3]) * 0.5f, y = (box[0] + box[2]) * 0.5f of
 * its box (ymin, xmin, ymax, xmax).  The person's root box is bbox[b][p][0], its root score score[b][p][0].
 *
 * One frame, all comparisons on the state as it was before the frame, every f32 step one IEEE operation rounded on its own
 * (no contraction, IEEE division):
 *   1 pair values    for a live slot i (id != 0) and a person p: with the areas a = (ymax - ymin) * (xmax - xmin) of the two
 *                    root boxes, tl = the larger ymin / xmin, br = the smaller ymax / xmax,
 *                    inter = ((br0 - tl0) * (br1 - tl1)) * [tl0 < br0 && tl1 < br1] and iou = inter / ((a_i + a_p) - inter)
 *                    as in ppn_nms; an iou that is not > 0 (a NaN included) counts as 0.0f.  r2 = (kp_gate * kp_gate) * a_i
 *                    with a_i the TRACK's root area; n_close = the number of k in 1..K-1 present in both with
 *                    dx * dx + dy * dy <= r2, dx = x_p - x_i, dy = y_p - y_i against the slot's stored (smoothed) centre.
 *                    The pair is eligible iff iou >= iou_thr || n_close >= min_close.
 *   2 match          for p = 0 .. D-1 ascending (descending root score): among the live slots not yet taken in this frame and
 *                    eligible with p, the one with the largest n_close, then the largest iou, then the lowest index, is
 *                    taken by p.
 *   3 update         a taken slot: root = the person's root box; for every k in 0..K-1 present in the person,
 *                    xy = old + alpha * (new - old) per coordinate if the slot had k and alpha != 1.0f, otherwise xy = new;
 *                    mask = the person's presence bits (the centres of cleared bits stay as they are); miss = 0; hits += 1.
 *   4 age            a live slot not taken: miss += 1, and when miss > max_age it is freed: id = mask = hits = miss = 0.
 *   5 births         the unmatched participating people with root score >= birth_thr, in ascending p, take the free slots
 *                    in ascending index (slots freed in step 4 included): id = ++last_id[s], root, mask and the centres of
 *                    the present keypoints from the person (raw), hits = 1, miss = 0.  Without a free slot the person stays
 *                    untracked and PPN_TRACK_FLAG_SLOT_OVERFLOW is set.  Ids are never reused.
 *   6 outputs        out_id  i32 [B][max_humans]        the track id of person p, -1 for everyone else (untracked people,
 *                                                       non-participants, rows >= P); every entry is written on every call
 *                    out_hits i32 [B][max_humans]       the slot's hits after the frame, 0 where out_id is -1
 *                    out_xy  f32 [B][max_humans][K][2]  or NULL; rows p < P only: a present keypoint of a tracked person
 *                                                       gets the slot's stored centre (x, y), anyone else's present
 *                                                       keypoint its raw centre, an absent keypoint (0, 0)
 *                    out_live i32 [B]                   the number of live slots after the frame
 *
 *   count i32 [B], kp_cell i32 [B][max_humans][K], bbox f32 [B][max_humans][K][4] (16-byte aligned), score f32
 *   [B][max_humans][K]: ppn_decode's outputs as they live on the device.
 * One launch on `stream` (one workgroup per stream), no allocation, no host synchronisation, no D2H: the call can be captured
 * into a graph.  No atomics -- each stream's workgroup owns its flags word, which it ORs into and the caller clears; two runs
 * give identical bytes.  PPN_E_INVALID before anything is launched for: a NULL cfg, st, state pointer, input or required
 * output; K outside 1..PPN_MAX_KP; min_close < 1; max_age < 0; a non-finite cfg value, iou_thr outside [0, 1], kp_gate < 0,
 * alpha outside (0, 1]; streams, frames or max_humans < 1; a bbox that is not 16-byte aligned.  PPN_E_UNSUPPORTED:
 * max_humans > PPN_MATCH_MAX_PEOPLE.  Precondition: the boxes are finite; otherwise the ids are unspecified, but no access
 * leaves the buffers.
 */
#define PPN_TRACK_SLOTS 64            /* live tracks per stream: one lane each */
#define PPN_TRACK_MAX_DET 256         /* people per image that take part */
#define PPN_TRACK_FLAG_DET_OVERFLOW 1
#define PPN_TRACK_FLAG_SLOT_OVERFLOW 2

typedef struct ppn_track_cfg {
    int32_t K;          /* keypoints, keypoint 0 = the instance (root) box      */
    int32_t min_close;  /* >= 1                                                  */
    int32_t max_age;    /* >= 0: frames a track survives unmatched               */
    float iou_thr;      /* [0,1]                                                 */
    float kp_gate;      /* >= 0: gate radius as a fraction of sqrt(track root area) */
    float birth_thr;    /* root score a person needs to start a track            */
    float alpha;        /* (0,1]: smoothing weight of the new observation        */
} ppn_track_cfg;

typedef struct ppn_track_state {      /* device pointers; ALL ZERO BYTES = a fresh tracker */
    int32_t* id;      /* [S][64]   0 = free slot                                 */
    int32_t* miss;    /* [S][64]                                                 */
    int32_t* hits;    /* [S][64]                                                 */
    uint32_t* mask;   /* [S][64]   bit k: keypoint k present                     */
    float* root;      /* [S][64][4]   (ymin,xmin,ymax,xmax), raw                 */
    float* xy;        /* [S][64][K][2] (x,y) centres, smoothed                   */
    int32_t* last_id; /* [S]       ids handed out so far; the next id is ++last_id */
    int32_t* flags;   /* [S]       OR of PPN_TRACK_FLAG_*, cleared by the caller  */
} ppn_track_state;

int ppn_track_update(const ppn_track_cfg* cfg, const ppn_track_state* st, const int32_t* count, const int32_t* kp_cell,
                     const float* bbox, const float* score, int32_t streams, int32_t frames, int32_t max_humans,
                     const int32_t* n_frames /* [S] or NULL = `frames` each */, int32_t* out_id, int32_t* out_hits,
                     float* out_xy /* or NULL */, int32_t* out_live, void* stream);

/*
 * Per-track skeleton clips on the device (no counterpart in the reference), csrc/clips.hip: the last T = cfg->length frames
 * of every tracked person's keypoints, kept as a ring per track id in up to PPN_CLIP_SLOTS resident clips per stream and
 * handed out as one f32 [3][T][K] tensor (planes x, y, score) per clip: what a skeleton-based action model takes.
 * ppn_clip_push consumes ppn_decode's people lists and ppn_track_update's out_id (and, if wanted, its out_xy);
 * ppn_clip_gather writes all clips of all streams.  tests/clips_ref.py restates the rules below in NumPy; kernels and
 * restatement agree on bytes.
 *
 * ppn_clip_push.  Batch layout and n_frames are ppn_track_update's: image b = s * frames + t is frame t of stream s, only
 * t < n_frames[s] is processed (a negative n_frames[s] counts as 0, NULL means `frames` each), the frames of a stream go in
 * ascending t within the call, and a stream without a processed frame keeps every state byte and its flags word.  out_row
 * i32 [B][max_humans] is fully written on every call, -1 in every entry of an image that is not processed.
 * One processed frame, with P = min(max(count[b], 0), max_humans) and r = pos[s]:
 *   a who takes part  person p < P takes part iff ids[b][p] > 0.  Keypoint k is present iff kp_cell[b][p][k] >= 0; a present
 *                     keypoint's values are x, y = xy[b][p][k] when xy is given (ppn_track_update's out_xy, smoothed),
 *                     otherwise the centre of its box, x = (box[1] + box[3]) * 0.5f, y = (box[0] + box[2]) * 0.5f, and
 *                     score = score[b][p][k].  An absent keypoint contributes (0, 0, 0) whatever the inputs hold there.
 *   b seen            a live slot (id != 0) whose id equals a participant's id: ring row r gets the person's three planes,
 *                     mask row r its presence bits, ref the person's root box bbox[b][p][0]; gap = 0, len = min(len + 1, T).
 *   c unseen          every other live slot: ring row r becomes all zero floats, mask row r 0; gap += 1,
 *                     len = min(len + 1, T); when gap > max_gap the slot is freed: id = gap = len = 0 (ref, mask and ring
 *                     keep their bytes: len guards them).  This is ppn_track_update's ageing rule: fed by a tracker with
 *                     max_age == max_gap, both reset together, the live ids after every frame are the tracker's.
 *   d births          the participants whose id no live slot holds, in ascending p, take the free slots in ascending index
 *                     (slots freed in step c included): id, gap = 0, len = 1, ref and row r as in step b.  Without a free
 *                     slot the person's out_row is -1 and PPN_CLIP_FLAG_SLOT_OVERFLOW is set.
 *   e outputs         out_row[b][p] = the person's slot, -1 for non-participants, overflow and rows >= P; then
 *                     pos[s] = (r + 1) % T.
 * Precondition: the positive ids of one image are distinct (the tracker's are); otherwise the result is unspecified, but no
 * access leaves the buffers.
 *
 * ppn_clip_gather.  Every byte of out f32 [S][64][3][T][K], out_id and out_len i32 [S][64] is written.  For slot (s, i):
 * out_id and out_len are the state's id and len; time step j of the output is ring row (pos[s] + j) % T and is valid iff the
 * slot is live and j >= T - len: the clip is chronological, its newest frame at j = T - 1, zero-padded on the left; invalid
 * steps and free slots are zeros.  PPN_CLIP_NORM_NONE copies the valid rows.  PPN_CLIP_NORM_ROOT takes, from the slot's ref,
 * cx = (ref[1] + ref[3]) * 0.5f, cy = (ref[0] + ref[2]) * 0.5f, h = ref[2] - ref[0], w = ref[3] - ref[1], s = h if h > w else
 * w, replaced by 1.0f unless s > 0 (a degenerate or inverted box, a NaN); a present keypoint becomes ((x - cx) / s,
 * (y - cy) / s, score), the subtraction and the IEEE division each rounded on its own, an absent one stays (0, 0, 0).  The
 * reference box is the newest SEEN root box of the clip, not each frame's own: motion inside the clip survives.
 *
 * Each entry point is one launch on `stream` (push: one workgroup per stream; gather: one per slot), no allocation, no host
 * synchronisation, no D2H: both can be captured into a graph.  No atomics -- each stream's workgroup owns its flags word,
 * which it ORs into and the caller clears; two runs give identical bytes.  PPN_E_INVALID before anything is launched for:
 * a NULL cfg, st, state pointer, input or output (only xy and n_frames may be NULL); K outside 1..PPN_MAX_KP; length outside
 * 1..PPN_CLIP_MAX_LEN; max_gap < 0; an unknown norm; streams, frames or max_humans < 1.  PPN_E_UNSUPPORTED: max_humans >
 * PPN_MATCH_MAX_PEOPLE.
 */
#define PPN_CLIP_SLOTS 64             /* clips per stream: as many as the tracker has tracks */
#define PPN_CLIP_MAX_LEN 256
#define PPN_CLIP_NORM_NONE 0
#define PPN_CLIP_NORM_ROOT 1
#define PPN_CLIP_FLAG_SLOT_OVERFLOW 1

typedef struct ppn_clip_cfg {
    int32_t K;        /* keypoints, keypoint 0 = the instance (root) box      */
    int32_t length;   /* T: frames per clip, 1..PPN_CLIP_MAX_LEN               */
    int32_t max_gap;  /* >= 0: frames a clip survives without its id           */
    int32_t norm;     /* PPN_CLIP_NORM_*: what ppn_clip_gather does to x and y */
} ppn_clip_cfg;

typedef struct ppn_clip_state {       /* device pointers; ALL ZERO BYTES = fresh */
    int32_t* id;      /* [S][64]        0 = free                                      */
    int32_t* gap;     /* [S][64]        frames since the id was last seen             */
    int32_t* len;     /* [S][64]        rows pushed since the slot was taken, <= T     */
    float* ref;       /* [S][64][4]     root box (ymin,xmin,ymax,xmax) of the newest SEEN frame */
    uint32_t* mask;   /* [S][64][T]     per ring row: bit k = keypoint k present; 0 = unseen frame */
    float* ring;      /* [S][64][T][3][K]  planes x, y, score                          */
    int32_t* pos;     /* [S]            the ring row the NEXT processed frame writes, 0..T-1 */
    int32_t* flags;   /* [S]            OR of PPN_CLIP_FLAG_*, cleared by the caller   */
} ppn_clip_state;

int ppn_clip_push(const ppn_clip_cfg* cfg, const ppn_clip_state* st, const int32_t* count, const int32_t* kp_cell,
                  const float* bbox, const float* score, const int32_t* ids, const float* xy /* or NULL */, int32_t streams,
                  int32_t frames, int32_t max_humans, const int32_t* n_frames /* [S] or NULL = `frames` each */,
                  int32_t* out_row /* [B][max_humans] */, void* stream);
int ppn_clip_gather(const ppn_clip_cfg* cfg, const ppn_clip_state* st, int32_t streams, float* out /* [S][64][3][T][K] */,
                    int32_t* out_id /* [S][64] */, int32_t* out_len /* [S][64] */, void* stream);

/*
 * Zones and counting lines on the device (no counterpart in the reference), csrc/zones.hip: how many people stand in a
 * polygon, who entered or left it, how long they have been there, and how many crossed a line segment in which direction.
 * ppn_zone_update consumes ppn_decode's people lists and ppn_track_update's out_id (and, if wanted, its out_xy), keeps up to
 * PPN_ZONE_SLOTS tracked ids per stream and writes per-frame and per-person outputs.  tests/zones_ref.py restates the rules
 * below in NumPy; kernel and restatement agree on bytes.
 *
 * Geometry is per stream (cameras differ), in the pixels of the people lists the call is given: zone z < zone_n[s] is the
 * polygon of zone_nv[s][z] vertices zone_xy[s][z][i] = (x, y), line l < line_n[s] the directed segment from A = (ax, ay) to
 * B = (bx, by) = line_xy[s][l].  The host validates the tables; the kernel clamps zone_n and line_n to 0..16 and a vertex
 * number to 0..8, so it never reads outside a table, and treats a zone of fewer than 3 vertices as empty.  The bits z >=
 * zone_n of `inside` and the words z >= zone_n of `dwell` are only ever cleared: reset a stream when its geometry changes.
 *
 * Batch layout and n_frames are ppn_track_update's: image b = s * frames + t is frame t of stream s, only t < n_frames[s] is
 * processed (a negative n_frames[s] counts as 0, NULL means `frames` each), the frames of a stream go in ascending t within
 * the call, and a stream without a processed frame keeps every state byte.  Every f32 step below is rounded on its own (no
 * contraction, IEEE division).  One processed frame, with P = min(max(count[b], 0), max_humans):
 *   a anchors   for person p < P the root box is bbox[b][p][0] = (ymin, xmin, ymax, xmax); ax = (xmin + xmax) * 0.5f; ay =
 *               (ymin + ymax) * 0.5f for PPN_ZONE_ANCHOR_CENTER, ymax for PPN_ZONE_ANCHOR_BOTTOM; with xy given (ppn_track_update's
 *               out_xy, smoothed) and anchor CENTER, (ax, ay) = xy[b][p][0].  The person is valid iff kp_cell[b][p][0] >= 0 and
 *               ax and ay are finite.  in_now[p] has bit z set iff the person is valid and the even-odd ray test puts the
 *               anchor into zone z: over the edges (i, j = i - 1 cyclic) toggle when (yi > ay) != (yj > ay) and
 *               ax < (xj - xi) * (ay - yi) / (yj - yi) + xi.
 *   b match     ppn_clip_push's steps a to d with `gap` and `max_gap`: the valid people with ids[b][p] > 0 take part, in
 *               ascending p; a participant continues the live slot (id != 0) that holds its id (the first p wins the slot's
 *               frame): the slot is SEEN, gap = 0; every other live slot is UNSEEN: gap += 1, and it is FREED when gap >
 *               max_gap; then the participants whose id no live slot held, in ascending p, take the free slots in ascending
 *               index (slots freed in this frame included): the slot is BORN, id = the id, gap = 0; without a free slot
 *               PPN_ZONE_FLAG_SLOT_OVERFLOW is set.
 *   c seen      with P0 = last, P1 = the person's anchor, in = inside: for every line l, side(P) = ((bx - ax_l) * (P.y - ay_l) -
 *               (by - ay_l) * (P.x - ax_l)) >= 0; if side(P0) != side(P1), e0 = cross(P1 - P0, A - P0), e1 = cross(P1 - P0,
 *               B - P0) with cross(u, v) = u.x * v.y - u.y * v.x, and the step crosses the segment iff (e0 <= 0 && e1 >= 0) ||
 *               (e0 >= 0 && e1 <= 0): forward if side(P1), backward otherwise; line_total and the frame's out_line count it.
 *               Zones z < zone_n: entered = in_now & ~in, exited = in & ~in_now; dwell[z] = dwell[z] + 1 (saturating at
 *               2^31 - 1) if the bit stays set, 1 if newly set, 0 if clear.  Then last = P1, inside = in_now.  A step is taken
 *               from the last frame the id was SEEN in, however many unseen frames lie between.
 *   d born      inside = in_now, every set bit counts as entered, dwell[z] = 1 for the set bits and 0 for the others (all
 *               16), last = the anchor; no line test.
 *   e unseen    a live slot that survives: dwell[z] += 1 (saturating) for its set bits z < zone_n: the person is taken to be
 *               still there.
 *   f freed     every set bit z < zone_n counts as exited; id = gap = inside = 0, dwell[z] = 0 (all 16); last keeps its bytes.
 *               Rules d and f keep zone_total[z].entered - zone_total[z].exited == the live slots with bit z after every frame.
 *   g outputs   out_slot[b][p] = the person's slot, -1 for everybody else and rows >= P; out_inside[b][p] = in_now[p] of every
 *               listed person, tracked or not, 0 for rows >= P; out_zone[b][z] = (occupancy: the listed people with bit z;
 *               entered and exited of this frame; loitering: the live slots after the frame with dwell[z] >= loiter);
 *               out_line[b][l] = (forward, backward) of this frame; zeros for z >= zone_n and l >= line_n.
 * Every output byte is written on every call; an image that is not processed gets -1 in out_slot and 0 elsewhere.
 * Precondition: the positive ids of one image are distinct (the tracker's are); otherwise the result is unspecified, but no
 * access leaves the buffers.
 *
 * One launch on `stream` (one workgroup per stream), no allocation, no host synchronisation, no D2H: it can be captured
 * into a graph.  No atomics -- each stream's workgroup owns its words; two runs give identical bytes.  PPN_E_INVALID before
 * anything is launched for: a NULL cfg, geom, st, table, state pointer, input or output (only xy and n_frames may be NULL); K
 * outside 1..PPN_MAX_KP; max_gap < 0; an unknown anchor; loiter < 1; streams, frames or max_humans < 1.  PPN_E_UNSUPPORTED:
 * max_humans > PPN_MATCH_MAX_PEOPLE.
 */
#define PPN_ZONE_SLOTS 64             /* tracked ids per stream: as many as the tracker has tracks */
#define PPN_ZONE_MAX 16               /* zones per stream    */
#define PPN_ZONE_MAX_VERT 8           /* vertices per zone   */
#define PPN_LINE_MAX 16               /* lines per stream    */
#define PPN_ZONE_FLAG_SLOT_OVERFLOW 1
#define PPN_ZONE_ANCHOR_CENTER 0      /* the centre of the root box (or the smoothed centre) */
#define PPN_ZONE_ANCHOR_BOTTOM 1      /* the middle of the root box's lower edge: the feet   */

typedef struct ppn_zone_geom {        /* device pointers, filled from the host */
    const int32_t* zone_n;   /* [S]                                   */
    const int32_t* zone_nv;  /* [S][16]                               */
    const float* zone_xy;    /* [S][16][8][2]  (x, y)                 */
    const int32_t* line_n;   /* [S]                                   */
    const float* line_xy;    /* [S][16][4]     (ax, ay, bx, by)       */
} ppn_zone_geom;

typedef struct ppn_zone_cfg {
    int32_t K;        /* keypoints, keypoint 0 = the instance (root) box       */
    int32_t max_gap;  /* >= 0: frames an id is held without being seen          */
    int32_t anchor;   /* PPN_ZONE_ANCHOR_*                                      */
    int32_t loiter;   /* >= 1: frames of dwell from which a person loiters      */
} ppn_zone_cfg;

typedef struct ppn_zone_state {       /* device pointers; ALL ZERO BYTES = fresh */
    int32_t* id;          /* [S][64]      0 = free                                           */
    int32_t* gap;         /* [S][64]      frames since the id was last seen                  */
    uint32_t* inside;     /* [S][64]      bit z: in zone z at the last update                */
    int32_t* dwell;       /* [S][64][16]  consecutive frames in zone z                       */
    float* last;          /* [S][64][2]   anchor (x, y) of the last frame the id was seen in */
    int32_t* zone_total;  /* [S][16][2]   (entered, exited) since the reset                  */
    int32_t* line_total;  /* [S][16][2]   (forward, backward) since the reset                */
    int32_t* flags;       /* [S]          OR of PPN_ZONE_FLAG_*, cleared by the caller       */
} ppn_zone_state;

int ppn_zone_update(const ppn_zone_cfg* cfg, const ppn_zone_geom* geom, const ppn_zone_state* st, const int32_t* count,
                    const int32_t* kp_cell, const float* bbox, const int32_t* ids, const float* xy /* or NULL */,
                    int32_t streams, int32_t frames, int32_t max_humans,
                    const int32_t* n_frames /* [S] or NULL = `frames` each */, int32_t* out_slot /* [B][max_humans] */,
                    uint32_t* out_inside /* [B][max_humans] */, int32_t* out_zone /* [B][16][4] */,
                    int32_t* out_line /* [B][16][2] */, void* stream);

/*
 * Re-identification by appearance on the device (no counterpart in the reference), csrc/reid.hip: a small integer colour
 * descriptor per person, read straight from the raw frame (ppn_people_descr), and a gallery per stream that gives every
 * person a PERSISTENT id which survives a change of track id when the appearance matches somebody recently lost
 * (ppn_reid_update).  tests/reid_ref.py restates both entries in NumPy; kernels and restatement agree on bytes.  Nothing here
 * claims an identification accuracy: the descriptor is a colour histogram and the default threshold of the Python layer a
 * guess, not a measurement.  Not built: a learned embedding, identities across streams, more than 128 entries per stream, a
 * motion model.
 *
 * ppn_people_descr: `src` is one raw surface as ppn_redact_yuv takes it (NV12, I420, YUYV and PPN_PIX_BGR24, any pitch and
 * plane alignment, frame f at f * frame_stride; matrix and full_range are checked but not used: no colour is converted),
 * roi i32 [F][R][4] = (y0, x0, h, w) and status i32 [F][R] the DEVICE tables ppn_people_rois writes -> descr u16
 * [F][R][PPN_DESCR_LEN] and valid i32 [F][R].  All integer, so the bytes do not depend on any order:
 *   judging     a slot is described iff status == PPN_ROI_OK and the rectangle is good by ppn_ingest_rois' rule: y0 >= 0,
 *               x0 >= 0, h >= 1, w >= 1, y0 + h <= height, x0 + w <= width, x0 and w even in a YUV format, y0 and h even in
 *               NV12 / I420.  The table is data the host never sees, so it is judged on the device, per workgroup and before
 *               any read.  Any other slot gets valid = 0 and an all-zero descriptor, and the surface is not read for it.
 *   samples     a fixed grid of PPN_DESCR_ROWS x PPN_DESCR_COLS points per rectangle, whatever its size: sample (i, j) is
 *               the source pixel y = y0 + ((2 i + 1) * h) / 192, x = x0 + ((2 j + 1) * w) / 64 (integer division).  A
 *               rectangle smaller than the grid repeats pixels; the largest index is (191 * h) / 192 < h.
 *   channels    YUV formats: (c0, c1, c2) = (Y, U, V) of the pixel, the chroma being the sample the pixel shares:
 *               (y >> 1, x >> 1) in NV12 / I420, (y, x >> 1) in YUYV.  BGR24: (c0, c1, c2) = (G, B, R).
 *   bins        8 per channel: c >> 5 for Y and the three BGR channels, (min(max(c, 64), 191) - 64) >> 4 for U and V.
 *   bands       band = i / 32: roughly head and shoulders, torso, legs of a "people" rectangle.
 *   descriptor  descr[band][channel][bin] = the number of the band's samples in the bin: 3 x 3 x 8 = PPN_DESCR_LEN counts;
 *               each (band, channel) histogram of a valid slot sums to 1024.  valid = 1.
 * Every entry of descr and valid is written on every call.  One workgroup per (frame, slot), one launch on `stream`, no
 * global atomics, no workspace, no allocation, no host synchronisation: it can be captured into a graph, and two runs give
 * identical bytes.  PPN_E_INVALID before any launch for: everything ppn_redact_yuv refuses of a single surface; a NULL roi,
 * status, descr or valid; max_rois < 1; frames < 1 or frames * max_rois > 65535.
 *
 * ppn_reid_update: the gallery.  Batch layout and n_frames are ppn_track_update's: image b = s * frames + t is frame t of
 * stream s, only t < n_frames[s] is processed (a negative n_frames[s] counts as 0, NULL means `frames` each), the frames of a
 * stream go in ascending t within the call, and a stream without a processed frame keeps every state byte and its flags
 * word.  The similarity of two descriptors is their histogram intersection, the sum of min(a[k], b[k]) over the 72 counts:
 * an integer in 0..PPN_REID_SIM_MAX.  descr [B][max_rois][72] and valid [B][max_rois] are ppn_people_descr's outputs with
 * F = B and R = max_rois, ids [B][max_humans] ppn_track_update's out_id.  One processed frame, with P = min(max(count[b], 0),
 * max_humans); person p < P TAKES PART iff ids[b][p] > 0 and HAS A DESCRIPTOR iff p < max_rois && valid[b][p] != 0; an
 * entry is LIVE iff pid != 0; all comparisons are made on the state as it was before the frame:
 *   1 bound    a live entry whose tid equals a participant's id: the person continues that pid, lost = 0.  With a
 *              descriptor: descr = the new one if n == 0, otherwise per count
 *              descr = (old * ((1 << shift) - 1) + new + ((1 << shift) >> 1)) >> shift; n = min(n + 1, 65535).  Without
 *              one descr and n keep their bytes.
 *   2 relink   the participants whose id no live entry holds and who have a descriptor, in ascending p (descending root
 *              score): the candidates are the live entries not bound in step 1, not yet claimed in this frame, with n > 0
 *              and min_lost <= lost <= memory.  The winner has the largest similarity, then the smallest lost, then the
 *              lowest index.  It is CLAIMED iff its similarity >= thr: tid = the person's id (the track id it held is
 *              forgotten), lost = 0, the descriptor blended and n counted as in step 1.
 *   3 age      every live entry neither bound nor claimed: lost += 1; when lost > memory it is FREED: pid = tid = lost =
 *              n = 0 (descr keeps its bytes: n == 0 guards them).
 *   4 births   the participants still without an entry, in ascending p, take the free entries in ascending index, the
 *              ones freed in step 3 included: pid = ++last_pid[s], tid = the id, lost = 0; descr = the person's and n = 1,
 *              or n = 0 without a descriptor.  Without a free entry the person's out_pid is -1 and
 *              PPN_REID_FLAG_SLOT_OVERFLOW is set.  Pids are never reused.
 *   5 outputs  out_pid[b][p] = the person's pid, -1 for non-participants, overflow and rows >= P; out_sim[b][p] = the
 *              similarity a person relinked with in step 2, -1 for everybody else; out_live[b] = the live entries after the
 *              frame.  An image that is not processed gets -1 everywhere.  Every entry is written on every call.
 * Invariant: after every frame the tids of a stream's live entries are distinct, hence the positive out_pid of an image are
 * distinct -- the precondition ppn_clip_push and ppn_zone_update put on ids, so out_pid can stand in for the tracker's ids.
 * Precondition: the positive ids of one image are distinct (the tracker's are); otherwise the result is unspecified, but no
 * access leaves the buffers.
 *
 * One launch on `stream` (one workgroup per stream), no allocation, no host synchronisation, no D2H, no atomics: it can be
 * captured into a graph and two runs give identical bytes.  PPN_E_INVALID before anything is launched for: a NULL cfg, st,
 * state pointer, input or output (only n_frames may be NULL); thr outside 0..PPN_REID_SIM_MAX; min_lost < 1; memory < 0;
 * shift outside 0..4; max_rois < 1; streams, frames or max_humans < 1.  PPN_E_UNSUPPORTED: max_humans > PPN_MATCH_MAX_PEOPLE.
 */
#define PPN_DESCR_ROWS 96             /* sample rows per rectangle                            */
#define PPN_DESCR_COLS 32             /* sample columns per rectangle                         */
#define PPN_DESCR_BANDS 3
#define PPN_DESCR_BINS 8
#define PPN_DESCR_LEN 72              /* 3 bands x 3 channels x 8 bins                        */
#define PPN_REID_SLOTS 128            /* gallery entries per stream                           */
#define PPN_REID_SIM_MAX 9216         /* 9 histograms of 1024 samples                         */
#define PPN_REID_FLAG_SLOT_OVERFLOW 1

int ppn_people_descr(const ppn_yuv_surface* src, int32_t frames, const int32_t* roi /* [F][R][4] */,
                     const int32_t* status /* [F][R] */, int32_t max_rois, uint16_t* descr /* [F][R][72] */,
                     int32_t* valid /* [F][R] */, void* stream);

typedef struct ppn_reid_cfg {
    int32_t thr;       /* 0..9216: the similarity from which a lost entry is taken up again   */
    int32_t min_lost;  /* >= 1: processed frames an entry must have been unseen for           */
    int32_t memory;    /* >= 0: processed frames an entry is kept unseen                      */
    int32_t shift;     /* 0..4: the new descriptor's weight in the blend is 2^-shift          */
    int32_t max_rois;  /* >= 1: the R of descr and valid                                      */
} ppn_reid_cfg;

typedef struct ppn_reid_state {       /* device pointers; ALL ZERO BYTES = fresh */
    int32_t* pid;        /* [S][128]      0 = free                                          */
    int32_t* tid;        /* [S][128]      the track id the entry is bound to                */
    int32_t* lost;       /* [S][128]      processed frames since it was seen                */
    int32_t* n;          /* [S][128]      descriptors blended in so far, at most 65535      */
    uint16_t* descr;     /* [S][128][72]                                                    */
    int32_t* last_pid;   /* [S]           the last pid handed out                           */
    int32_t* flags;      /* [S]           OR of PPN_REID_FLAG_*, cleared by the caller      */
} ppn_reid_state;

int ppn_reid_update(const ppn_reid_cfg* cfg, const ppn_reid_state* st, const int32_t* count /* [B] */,
                    const int32_t* ids /* [B][max_humans] */, const uint16_t* descr /* [B][max_rois][72] */,
                    const int32_t* valid /* [B][max_rois] */, int32_t streams, int32_t frames, int32_t max_humans,
                    const int32_t* n_frames /* [S] or NULL = `frames` each */, int32_t* out_pid /* [B][max_humans] */,
                    int32_t* out_sim /* [B][max_humans] */, int32_t* out_live /* [B] */, void* stream);

/*
 * Actions from skeleton clips (no counterpart in the reference), csrc/stgcn.hip: the forward pass of ST-GCN (Yan, Xiong,
 * Lin 2018), one person per clip, eval mode, exact f32, on what ppn_clip_gather wrote.  tests/stgcn_ref.py restates the
 * function from the unfolded state dict; actions.py folds every BatchNorm and bias on the host (f64, rounded once).
 *
 * Layout.  `capacity` = streams * PPN_CLIP_SLOTS clips at most.  The n = *n_active ACTIVE clips lie first in every activation
 * buffer, f32 [n][t][v][c], channels last; what follows them is never read or written.  All four entry points launch for the
 * capacity and read *n_active on the device: a workgroup whose clip index is >= *n_active exits at once, so a captured
 * graph replays on any population, zero included.  One output element is summed in one fixed order that depends on nothing
 * but the descriptor: a clip's values do not depend on the other clips or on its place in the list.  No atomics.
 *
 * ppn_stgcn_input (uses dtype, K, T).  Slot j = s * 64 + i of x f32 [S][64][3][T][K], ids and length i32 [S][64] is ACTIVE
 * iff ids[j] != 0 && length[j] >= min_len.  With r(j) the number of active slots before j: rank[j] = r(j) if active else
 * -1; active[r(j)] = j; active[m] = -1 for m >= n; *n_active = n.  Every byte of active i32 [S*64], rank i32 [S*64] and
 * n_active is written.  For an active slot x0[r][t][v][c] = fmaf(x[j][c][t][v], scale[v*3+c], shift[v*3+c]) (data_bn
 * folded; zero-padded frames are not special-cased).
 *
 * ppn_stgcn_gcn.  x [n][T][K][cin] -> out [n][T][K][cout]:
 *   y[t][w][p][ci] = sum_v x[t][v][ci] * adj[p][v][w]          (MFMA: an fmaf chain from 0, v ascending, zeros past K; adj
 *                                                                f32 [P][K][K] already multiplied by the edge importance)
 *   z[t][w][c]     = sum_{ci chunk of 16} sum_p sum_{ci in chunk} W[p*cout+c][ci] * y[t][w][p][ci]     (MFMA, chunks ascending)
 *   out            = max(fmaf(z, s0[c], t0[w][c]), 0)          t0 f32 [K][cout] carries the gcn bias passed through adj
 * cin is padded to a multiple of 16 inside the kernel (x is read with its own pitch cin; the packed weights hold zeros).
 * w is packed in fragment order: float4 number ((ct * ncc + cc) * P + p) * 64 + g * 16 + col, component j, is
 * W[p*cout + ct*16 + col][cc*16 + 4*g + j], ct < cout/16, cc < ncc = ceil(cin/16), zero where the input channel is >= cin.
 *
 * ppn_stgcn_tcn.  u [n][T][K][cout] (the gcn's output), x [n][T][K][cin] (the block's input; NULL for PPN_STGCN_RES_NONE)
 * -> out [n][To][K][cout], To = (T - 1) / stride + 1:
 *   z[t'][v][c] = sum_{ci chunk} sum_{k<9} sum_{ci} Wt[c][ci][k] * u[t'*stride - 4 + k][v][ci]
 *                 (+ sum_{ci chunk} sum_{ci} Wr'[c][ci] * x[t'*stride][v][ci]   for PPN_STGCN_RES_PROJ, Wr' = Wr * sr / s3)
 *   out         = max(fmaf(z, s3[c], t3[c]) (+ x[t'][v][c] for PPN_STGCN_RES_IDENTITY), 0)
 * A tap whose time step lies outside [0, T) OF ITS OWN CLIP contributes zero.  w: float4 number ((ct * ncc + cc) * 9 + k) *
 * 64 + g * 16 + col, component j, is Wt[ct*16 + col][cc*16 + 4*g + j][k], ncc = cout/16; behind these (cout/16) * ncc * 9 *
 * 64 float4, for PROJ, float4 number (ct * nrc + rc) * 64 + g * 16 + col is Wr'[ct*16 + col][rc*16 + 4*g + j], nrc =
 * ceil(cin/16), zero past cin.
 *
 * ppn_stgcn_head (uses dtype, K, T = the last block's To, cout = its channels).  For slot j with r = rank[j] >= 0:
 * pooled[c] = (sum over (t, v) ascending of x[r][t][v][c]) / (T*K); logits[j][m] = fmaf chain over c ascending from b[m] with
 * w f32 [c][num_class]; label[j] = the lowest index of the largest logit.  rank[j] < 0: zeros and -1.  Every byte of logits
 * f32 [S][64][num_class] and label i32 [S][64] is written.
 *
 * Each entry point is one launch on `stream`, no allocation, no host synchronisation, no D2H.  PPN_E_UNSUPPORTED before any
 * launch: dtype != PPN_F32 (PPN_F16: ppn_stgcn16_* below).  PPN_E_INVALID: a NULL descriptor or pointer (x of the tcn may be
 * NULL without a shortcut); K outside 1..PPN_MAX_KP; T outside 1..PPN_CLIP_MAX_LEN; P outside 1..PPN_STGCN_MAX_P; cout not a
 * multiple of 16 in 16..PPN_STGCN_MAX_C; cin neither 3 nor such a multiple; stride not 1 or 2; an unknown residual; an
 * identity shortcut with cin != cout or stride 2; num_class outside 1..PPN_STGCN_MAX_CLASS; streams outside
 * 1..PPN_STGCN_MAX_STREAMS; a capacity that is not streams * 64; a weight, scale, shift or activation pointer the kernels
 * read or write as float4 that is not 16-byte aligned.
 */
#define PPN_STGCN_MAX_P 3
#define PPN_STGCN_MAX_C 256
#define PPN_STGCN_MAX_CLASS 1024
#define PPN_STGCN_MAX_STREAMS 1024
#define PPN_STGCN_RES_NONE 0
#define PPN_STGCN_RES_IDENTITY 1
#define PPN_STGCN_RES_PROJ 2

typedef struct ppn_stgcn_desc {
    int32_t dtype;     /* PPN_F32 for ppn_stgcn_*, PPN_F16 for ppn_stgcn16_*                  */
    int32_t K;         /* joints                                                       */
    int32_t P;         /* partitions of the adjacency, 1..3                            */
    int32_t T;         /* time steps of the stage's input                              */
    int32_t cin;       /* the block's input channels: 3 or a multiple of 16            */
    int32_t cout;      /* the block's output channels: a multiple of 16, <= 256        */
    int32_t stride;    /* temporal stride of the block: 1 or 2                         */
    int32_t residual;  /* PPN_STGCN_RES_*                                              */
} ppn_stgcn_desc;

int ppn_stgcn_input(const ppn_stgcn_desc* d, const float* x /* [S][64][3][T][K] */, const int32_t* ids, const int32_t* length,
                    int32_t streams, int32_t min_len, const float* scale /* [K*3] */, const float* shift /* [K*3] */,
                    int32_t* active /* [S*64] */, int32_t* n_active /* [1] */, int32_t* rank /* [S*64] */,
                    float* x0 /* [S*64][T][K][3] */, void* stream);
int ppn_stgcn_gcn(const ppn_stgcn_desc* d, const float* x, const float* w, const float* adj /* [P][K][K] */,
                  const float* s0 /* [cout] */, const float* t0 /* [K][cout] */, const int32_t* n_active, int32_t capacity,
                  float* out, void* stream);
int ppn_stgcn_tcn(const ppn_stgcn_desc* d, const float* u, const float* x /* or NULL */, const float* w,
                  const float* s3 /* [cout] */, const float* t3 /* [cout] */, const int32_t* n_active, int32_t capacity,
                  float* out, void* stream);
int ppn_stgcn_head(const ppn_stgcn_desc* d, int32_t num_class, const float* x, const float* w /* [c][num_class] */,
                   const float* b /* [num_class] */, const int32_t* rank /* [S*64] */, int32_t streams,
                   float* logits /* [S][64][num_class] */, int32_t* label /* [S][64] */, void* stream);

/*
 * The same forward pass with IEEE half storage, csrc/stgcn16.hip: v_mfma_f32_16x16x32_f16 with f32 accumulation.  The four
 * entry points take the ppn_stgcn_desc with dtype == PPN_F16 and the argument lists of their f32 counterparts; activations and
 * packed weights are IEEE half behind void pointers; the scale and shift tables (scale, shift, s0, t0, s3, t3), the
 * classifier's w and b and the logits stay f32.  The layout, launch and determinism rules above hold unchanged: one launch per
 * entry point for the capacity, *n_active read on the device, a workgroup past it exits at once, no allocation, no
 * synchronisation, no read-back, no atomics, no split reductions; one output element is summed in one fixed order that depends
 * on nothing but the descriptor, so a clip's bits depend neither on the other clips nor on its place.  tests/stgcn16_ref.py
 * restates the mode.  "half(v)" is ONE rounding of the f32 value v to nearest even.
 *
 * Range.  Conversions do not clamp: a value beyond 65504 becomes inf, and from there on the clip's results are inf or NaN.
 * ActionModel.half_range_report tells whether a checkpoint's activations fit.
 *
 * Depth lanes past the data.  The MFMA's depth step is 32.  A depth lane or row that the data does not cover (a joint
 * v >= K, a channel >= cin or cout, the pad channel of x0) takes the value 0 in BOTH operands, never what lies behind the row
 * in memory or LDS: stale half bits can be inf or NaN, and 0 * inf poisons the sum.
 *
 * ppn_stgcn16_input.  active, rank and n_active are byte for byte what ppn_stgcn_input writes.  x0 is half [n][T][K][4]:
 * x0[r][t][v][c] = half(fmaf(x[j][c][t][v], scale[v*3+c], shift[v*3+c])) for c < 3, computed in f32; x0[r][t][v][3] = 0, so
 * rows are 8 bytes.  A block with cin == 3 (its graph convolution, and a projection shortcut from it) reads its input with
 * this pitch of 4; every other block with its pitch cin.
 *
 * Weights and adjacency.  adj half [P][K][K] is the adjacency already multiplied by the edge importance; it and every packed
 * weight (W, Wt, Wr' = Wr * sr / s3) are rounded ONCE from the f64 folded value to half, on the host.  A 16-byte unit holds the
 * 8 halves j = 0..7 of one lane's A fragment, lane = g * 16 + col:
 *   gcn w:  unit ((ct * ncc + cc) * P + p) * 64 + g * 16 + col, half j, is W[p*cout + ct*16 + col][cc*32 + 8*g + j],
 *           ct < cout/16, cc < ncc = ceil(cin/32), zero where the input channel is >= cin.
 *   tcn w:  unit ((ct * ncc + cc) * 9 + k) * 64 + g * 16 + col, half j, is Wt[ct*16 + col][cc*32 + 8*g + j][k], ncc =
 *           ceil(cout/32), zero where the input channel is >= cout; behind these (cout/16) * ncc * 9 * 64 units, for PROJ, unit
 *           (ct * nrc + rc) * 64 + g * 16 + col, half j, is Wr'[ct*16 + col][rc*32 + 8*g + j], nrc = ceil(cin/32), zero past cin.
 *
 * ppn_stgcn16_gcn.  x half [n][T][K][cin or 4] -> out half [n][T][K][cout]:
 *   y[t][w][p][ci] = half(sum_v x[t][v][ci] * adj[p][v][w])     (one MFMA over the joints, f32 accumulation, zeros past K)
 *   z[t][w][c]     = sum_{ci chunk of 32} sum_p sum_{ci in chunk} W[p*cout+c][ci] * y[t][w][p][ci]      (MFMA, f32 accumulation,
 *                                                                 chunks ascending, p ascending inside a chunk)
 *   out            = half(max(fmaf(z, s0[c], t0[w][c]), 0))
 *
 * ppn_stgcn16_tcn.  u half [n][T][K][cout], x half [n][T][K][cin or 4] (NULL for PPN_STGCN_RES_NONE) -> out half
 * [n][To][K][cout]: z as in ppn_stgcn_tcn, accumulated in f32 over chunks of 32 channels ascending, the nine taps ascending
 * inside a chunk, then the projection shortcut's chunks; o = fmaf(z, s3[c], t3[c]) in f32 (+ float(x[t'][v][c]) in f32 for
 * PPN_STGCN_RES_IDENTITY); out = half(max(o, 0)).  A tap whose time step lies outside [0, T) OF ITS OWN CLIP contributes zero.
 *
 * ppn_stgcn16_head.  ppn_stgcn_head reading half x: pooled in f32 in the same order, the same classifier and arg-max; every
 * byte of logits f32 [S][64][num_class] and label i32 [S][64] is written.
 *
 * PPN_E_UNSUPPORTED before any launch: dtype != PPN_F16 (PPN_F32 and PPN_BF16 included).  PPN_E_INVALID: everything
 * ppn_stgcn_* refuses so, and an x0, x, u, w, s0, t0, s3, t3 or out pointer (x of the tcn: with a shortcut) that is not 16-byte
 * aligned.
 */
int ppn_stgcn16_input(const ppn_stgcn_desc* d, const float* x /* [S][64][3][T][K] */, const int32_t* ids, const int32_t* length,
                      int32_t streams, int32_t min_len, const float* scale /* [K*3] */, const float* shift /* [K*3] */,
                      int32_t* active /* [S*64] */, int32_t* n_active /* [1] */, int32_t* rank /* [S*64] */,
                      void* x0 /* half [S*64][T][K][4] */, void* stream);
int ppn_stgcn16_gcn(const ppn_stgcn_desc* d, const void* x, const void* w, const void* adj /* half [P][K][K] */,
                    const float* s0 /* [cout] */, const float* t0 /* [K][cout] */, const int32_t* n_active, int32_t capacity,
                    void* out, void* stream);
int ppn_stgcn16_tcn(const ppn_stgcn_desc* d, const void* u, const void* x /* or NULL */, const void* w,
                    const float* s3 /* [cout] */, const float* t3 /* [cout] */, const int32_t* n_active, int32_t capacity,
                    void* out, void* stream);
int ppn_stgcn16_head(const ppn_stgcn_desc* d, int32_t num_class, const void* x, const float* w /* [c][num_class] */,
                     const float* b /* [num_class] */, const int32_t* rank /* [S*64] */, int32_t streams,
                     float* logits /* [S][64][num_class] */, int32_t* label /* [S][64] */, void* stream);

/*
 * The monitoring overlay (no counterpart in the reference), csrc/render.hip: track ids, zones, counting lines and their
 * counts painted by the rasteriser of ppn_draw_humans, onto RGB frames (ppn_draw_scene) or raw NV12 / I420 / YUYV surfaces
 * (ppn_draw_scene_yuv), from ppn_track_update's and ppn_zone_update's results as they lie on the device: nothing is read
 * back, and the colours of a zone or line follow this frame's occupancy and crossings.  tests/overlay_ref.py restates the
 * rules below in NumPy; kernel and restatement agree on every byte.  Not built: alpha-blended zone fill, trails, text other
 * than the 16 glyphs.
 *
 * The picture is ppn_draw_humans' (resp. ppn_draw_humans_yuv's) with a second list of primitives per image painted after
 * all people and before the grid; everything else -- the surface rule, in place / out of place, pitches, limits -- is
 * theirs.  Image b = s * frames + t is frame t of stream s (ppn_track_update's layout); an image with t >= n_frames[s]
 * gets no overlay (NULL n_frames: every image is processed).  The list has a fixed slot per item, the slot order being the
 * paint order: zone z = 0..15 (edges 0..7, plate, text), then line l = 0..15 (segment, tick, plate, text), then person
 * p = 0 .. min(count, max_humans) - 1 (root outline, plate, text).  T is truncation toward zero of an f32; a value v is
 * usable iff |v| < 2^20 (NaN is not); every f32 step is one IEEE operation rounded on its own.
 *
 * Primitives (NORMATIVE).  A line is ppn_draw_humans' limb: PIL's width-2 line between integer end points, one pixel for a
 * zero vector.  A fill is the inclusive pixel box [x0, y0, x1, y1].  A text is n <= 16 glyphs of the font below at (x0, y0)
 * with scale s: pixel (x, y) is covered iff, with u = x - x0, v = y - y0 (integer division): u >= 0, 0 <= v < 7 s,
 * c = u / (6 s) < n, col = (u % (6 s)) / s < 5, and bit 4 - col of FONT[code_c][v / s] is set.  A label at (x0, y0) is the
 * plate, the fill [x0 - 1, y0 - 1, x0 + 6 s n - s, y0 + 7 s] in `plate`, drawn only when cfg.plates is set, and then the
 * text in `text`.  Numbers are decimal without leading zeros; a count v is printed as min(max(v, 0), 999999), an id in
 * full.  The font, seven row bytes per glyph code from the top row down, bit 4 the leftmost column:
 *     FONT  0   0E 11 13 15 19 11 0E     '0'
 *     FONT  1   04 0C 04 04 04 04 0E     '1'
 *     FONT  2   0E 11 01 02 04 08 1F     '2'
 *     FONT  3   1F 02 04 02 01 11 0E     '3'
 *     FONT  4   02 06 0A 12 1F 02 02     '4'
 *     FONT  5   1F 10 1E 01 01 11 0E     '5'
 *     FONT  6   06 08 10 1E 11 11 0E     '6'
 *     FONT  7   1F 01 02 04 08 08 08     '7'
 *     FONT  8   0E 11 11 0E 11 11 0E     '8'
 *     FONT  9   0E 11 11 0F 01 02 0C     '9'
 *     FONT 10   00 04 04 00 04 04 00     ':'
 *     FONT 11   00 00 00 1F 00 00 00     '-'
 *     FONT 12   0A 0A 1F 0A 1F 0A 0A     '#'
 *     FONT 13   00 00 00 00 00 00 00     ' '
 *     FONT 14   00 00 00 00 00 00 00     spare
 *     FONT 15   00 00 00 00 00 00 00     spare
 *
 * The zone part (all of geom's tables, out_zone, out_line and line_total given; all NULL: no zone part).  zone_n and line_n
 * are clamped to 0..16 and a vertex number nv to 0..8 as ppn_zone_update clamps them.
 *   zone z     drawn iff z < zone_n[s], nv >= 3 and every coordinate of its nv vertices is usable.  Edge i < nv: the line
 *              from (T(x_i), T(y_i)) to (T(x_j), T(y_j)), j = (i + 1) mod nv, in `alert` if out_zone[b][z][3] > 0 (somebody
 *              loiters), else `active` if out_zone[b][z][0] > 0 (occupied), else zone_colour[z].  Label: the occupancy
 *              out_zone[b][z][0] at (T(x_0) + 3, T(y_0) + 3).
 *   line l     drawn iff l < line_n[s] and ax, ay, bx, by are usable.  Colour: `active` if out_line[b][l][0] +
 *              out_line[b][l][1] > 0 (wrapping i32), else line_colour[l].  Segment: the line from (T(ax), T(ay)) to
 *              (T(bx), T(by)).  Tick, on the side a forward crossing ends on: dx = bx - ax, dy = by - ay,
 *              len = sqrtf(dx * dx + dy * dy), mx = (ax + bx) / 2, my = (ay + by) / 2, q = tick / len,
 *              ex = mx + (-dy) * q, ey = my + dx * q: the line from (T(mx), T(my)) to (T(ex), T(ey)); omitted when
 *              len == 0 or ex or ey is not usable.  Label "F:B" at (T(mx) + 3, T(my) + 3), the cumulative totals AS OF
 *              THIS FRAME: F = line_total[s][l][0] - the sum over t' > t of out_line[s * frames + t'][l][0] in wrapping
 *              i32 arithmetic, B likewise on [1].  line_total holds the totals after the whole batch; taking the later
 *              frames' crossings off again gives each frame of a batch of several frames per stream its own running
 *              count, so the numbers on consecutive frames step when the crossing happens, not at the batch's start.
 * The id part (ids given; NULL: no id part).  Person p < min(max(count[b], 0), max_humans) with ids[b][p] > 0 whose root
 * keypoint takes part in ppn_draw_humans' picture (kp_cell[b][p][0] >= 0, its four box values usable): the root's two
 * outlines again, in id_colour[id & 15], and the id as a label at x0 = T(xmin), y0 = T(ymin) - 7 s - 1, or, when
 * y0 - 1 < 0 (the plate would leave the frame at the top), at y0 = T(ymin) + 3, inside the box.
 * With neither part the call is ppn_draw_humans (ppn_draw_humans_yuv).
 *
 * workspace: ppn_draw_scene_workspace_bytes(cfg, batch, max_humans) bytes, 16-byte aligned: the people's records and 48
 * bytes per overlay slot (224 + 3 max_humans per image) behind them.  Still two launches on `stream` -- one setup kernel
 * writes both lists --, no allocation, no host synchronisation: capturable into a graph.  For a raw surface the overlay's
 * colours are converted on the host with ppn_rgb_to_yuv's rule, like the palette.  PPN_E_INVALID before any launch:
 * everything ppn_draw_humans (ppn_draw_humans_yuv) refuses; a NULL overlay or in; scale outside 1..4; frames < 1; batch no
 * multiple of frames; a negative or non-finite tick; some but not all pointers of the zone part.
 */
typedef struct ppn_overlay_cfg {
    int32_t frames;                  /* frames per stream in the batch, >= 1 */
    int32_t scale;                   /* glyph pixel size s, 1..4            */
    float tick;                      /* length of a line's direction tick in pixels, finite, >= 0 */
    int32_t plates;                  /* draw the plates under the texts     */
    uint8_t zone_colour[16][4], line_colour[16][4], id_colour[16][4];        /* r, g, b, unused */
    uint8_t active[4], alert[4], text[4], plate[4];
} ppn_overlay_cfg;

typedef struct ppn_overlay_in {      /* device pointers */
    const int32_t* ids;              /* [B][max_humans]  ppn_track_update's out_id, or NULL                     */
    ppn_zone_geom geom;              /* the tables ppn_zone_update was given                                    */
    const int32_t* out_zone;         /* [B][16][4]       ppn_zone_update's outputs of this batch                */
    const int32_t* out_line;         /* [B][16][2]                                                              */
    const int32_t* line_total;       /* [S][16][2]       ppn_zone_state.line_total after that update            */
    const int32_t* n_frames;         /* [S] or NULL                                                             */
} ppn_overlay_in;

size_t ppn_draw_scene_workspace_bytes(const ppn_draw_cfg* cfg, int32_t batch, int32_t max_humans); /* 0 on a bad argument */
int ppn_draw_scene(const ppn_draw_cfg* cfg, const ppn_overlay_cfg* overlay, const ppn_overlay_in* in, const uint8_t* src,
                   uint8_t* dst, int32_t batch, int32_t height, int32_t width, const int32_t* count, const int32_t* kp_cell,
                   const float* bbox, int32_t max_humans, void* workspace, void* stream);
int ppn_draw_scene_yuv(const ppn_draw_cfg* cfg, const ppn_overlay_cfg* overlay, const ppn_overlay_in* in,
                       const ppn_yuv_surface* src, const ppn_yuv_surface* dst, int32_t batch, const int32_t* count,
                       const int32_t* kp_cell, const float* bbox, int32_t max_humans, void* workspace, void* stream);

/*
 * Horizontal-flip test-time averaging (no counterpart in the reference), csrc/tta.hip: the network sees a frame and its
 * left-right mirror image, the second head is mapped back and averaged with the first, and only then the decode runs.
 * Geometry as in ppn_decode_cfg; the heads are f32 [batch, C, H, W] NCHW with C = 6K + E*sH*sW: six unary groups resp, conf,
 * x, y, w, h of K channels each, then e[E][sH][sW] (limb channel e_chan(e, ly, lx) = 6K + (e*sH + ly)*sW + lx).
 *   kp_mirror[k]     the keypoint whose name has left_ / right_ swapped, k itself where there is no such prefix;
 *   edge_mirror[e]   the edge (kp_mirror[src], kp_mirror[dst]).  Both must be involutions of [0, K) / [0, E).
 * With A the head of the frame and Bm the head of the mirrored frame, mirror(Bm) is, per image, at cell (i, j):
 *   groups resp, conf, y, w, h    Bm[g, kp_mirror[k], i, W-1-j]
 *   group x                       1.0f - Bm[x, kp_mirror[k], i, W-1-j]
 *   limbs                         Bm[e_chan(edge_mirror[e], ly, sW-1-lx), i, W-1-j]
 * and the merged head is M = (A + mirror(Bm)) * 0.5f elementwise in f32: one IEEE addition, then one multiplication, no
 * contraction, no reassociation, subnormals kept -- NumPy's ((a + m) * np.float32(0.5)) bit for bit (tests/tta_ref.py).
 * Precondition: inputs in [0, 1] (sigmoid outputs); the result for NaNs or negative values is unspecified.
 */
typedef struct ppn_tta_cfg {
    int32_t K, E, sH, sW, H, W;            /* as in ppn_decode_cfg */
    int32_t kp_mirror[PPN_MAX_KP];
    int32_t edge_mirror[PPN_MAX_EDGES];
} ppn_tta_cfg;

/*
 * Reads head_a (A) and head_b (Bm) once and writes what ppn_decode_fused takes:
 *   out_unary  f32 [batch, 6K, H, W]   the first 6K channels of M
 *   out_keys   u64 [batch, E, H, W]    (uint64)float_bits(max_s M[e, s, cell]) << 32 | ~(uint32)s_first, with s = ly*sW + lx
 *                                      in MERGED order and s_first the lowest s attaining the maximum (the key format of
 *                                      ppn_conv_desc.argmax_keys)
 *   out_head   f32 [batch, C, H, W] or NULL: M in full, written only when given; must not overlap head_a / head_b
 * One unary launch and one limb launch on `stream`; no allocation, no host synchronisation, no memset node.  When the
 * window is split across workgroups the unary launch clears out_keys and the slices are combined by a u64 atomic maximum:
 * the largest value, then the lowest s, in any order, so two runs give identical bytes.  The environment knob PPN_TTA_SPLIT = n, read at
 * every call, sets the number of window slices per (edge, image) (default: chosen from batch so that the grid fills the GPU);
 * results do not depend on it.  PPN_E_INVALID before anything is launched for: a NULL cfg / head_a / head_b / out_unary /
 * out_keys, K outside 1..PPN_MAX_KP, E outside 0..PPN_MAX_EDGES, a non-positive window, grid or batch, a mirror table that
 * indexes out of range or is not an involution, an output overlapping an input, a misaligned pointer.
 */
int ppn_tta_merge(const ppn_tta_cfg* cfg, const float* head_a, const float* head_b, int32_t batch, float* out_unary,
                  uint64_t* out_keys, float* out_head, void* stream);

/*
 * The doubled batch of a flip-averaged forward: dst holds 2 * rows rows of `width` elements of elem_bytes bytes; its first
 * `rows` rows are a copy of src, row rows + r is row r of src with its elements in reverse order.
 *   elem_bytes 3   u8 [B,H,W,3] RGB frames: rows = B*H, width = W     (dst = a plan's u8 input buffer of batch 2B)
 *   elem_bytes 4   f32 [B,3,H,W] inputs:    rows = B*3*H, width = W   (4-byte aligned)
 * dst must not overlap src.  One launch on `stream`; rows = 0 is a no-op.
 */
int ppn_tta_stage(const void* src, void* dst, int64_t rows, int32_t width, int32_t elem_bytes, void* stream);

/* Process-wide tile choice of the large-tile convolution kernel.  0 (default): one launch at a time -- tiles are
 * sized so that the workgroup count fills whole rounds of the 256 CUs.  1: several launches are in flight on
 * different streams (rt.MultiLaneInference) -- a partial last round is filled by the other stream's workgroups, so
 * the most efficient tile shape is taken regardless of the round count (measured +4..5 % with two lanes). */
/* 2: as 0, plus two-segment launches where ppn_conv_split cuts (opt-in: measured 2-4 % slower end to end because the
 * single round of small tiles is slower than modelled; conv_big.hip::big_split_for has the numbers). */
int ppn_set_conv_tile_policy(int32_t policy);

/* Force the (pixels x channels) tile of the large-tile convolution kernel for every later launch / plan entry whose
 * Cout class admits it: bp in {128,192,256}, bc in {64,128,256} (not 192x64); (0,0) restores the automatic choice.
 * Test and tuning hook: the automatic choice depends on B*Ho*Wo, so small parity problems would otherwise never
 * reach the instantiations a batch-32 384x384 forward runs (tests/test_conv_tiles_gpu.py).  Process-wide, like the
 * PPN_CONV_TILE="bp,bc" environment knob that supplies its initial value. */
int ppn_set_conv_tile_override(int32_t bp, int32_t bc);

/* Test and tuning hook: 0 routes the 64 -> 64 3x3 stride-1 convolutions of the 16-bit modes through the generic
 * implicit-GEMM kernels instead of the register-resident filter-bank kernel (csrc/conv64.hip); results are bit-identical
 * either way (tests/test_conv_tiles_gpu.py).  Process-wide; initial value 1 unless PPN_CONV64=0 is in the environment.
 * Product code uses ppn_conv_desc.flags (PPN_CONV_NO_FILTER_BANK) per descriptor / plan instead. */
int ppn_set_conv64_enabled(int32_t on);

/* Name of the kernel instantiation the calling thread's last successful ppn_conv2d_fused launched
 * (e.g. "conv_igemm_big_kernel<__bf16, 192, 256, 8, false>"); "" before the first call. */
const char* ppn_last_conv_kernel(void);

/* Strip loader of the large-tile kernel's 192 x 256 tile (csrc/conv_big.hip, template flag SP): 3x3 stride-1 "same"
 * convolutions of the 16-bit modes whose 192-pixel tiles are whole image rows stage one activation strip per filter row
 * instead of one stage per tap; results are bit-identical (tests/test_conv_strip_gpu.py).  ppn_last_conv_kernel() reports
 * the tile's name either way; ppn_last_conv_strip() is 1 iff the calling thread's last successful ppn_conv2d_fused took
 * the strip loader.  ppn_set_conv_strip_enabled: process-wide switch for every later launch and plan run (test and A/B
 * hook); initial value 1 unless PPN_CONV_STRIP=0 is in the environment. */
int ppn_last_conv_strip(void);
int ppn_set_conv_strip_enabled(int32_t on);

/*
 * First layer (drn.py:123-128 layer0: 7x7 conv 3->16, BN, ReLU) with the input normalisation of
 * rt_test.py:97-101 / aug.py:149-153 fused into the load.
 *   src      u8  [B,H,W,3]  RGB frame (src_is_u8=1): (x-mean_c)/std_c applied on the fly, or
 *            f32 [B,3,H,W]  already normalised NCHW input, the model.forward() argument (src_is_u8=0)
 *   weight   f32 [16,3,7,7] (reference layout, device), scale/shift f32[16] folded BN (device); both NULL =
 *            train mode: the plain convolution output is written (no affine, no ReLU)
 *   mean,std_ HOST pointers to 3 floats (read at call time; may be NULL when src_is_u8=0)
 *   out      NHWC [B,H,W,16] dtype
 */
int ppn_stem7x7(int32_t dtype, int32_t src_is_u8, const void* src, int32_t batch, int32_t h, int32_t w,
                const float* weight, const float* scale, const float* shift, const float* mean, const float* std_,
                void* out, void* stream);

/*
 * layer0 + layer1 (drn.py:123-130) in one launch: as ppn_stem7x7, then 3x3 conv 16->16 + BN + ReLU on the tile that
 * is still in LDS; the 16-channel tensor between the two layers never goes to HBM.
 *   w1 f32 [16,16,3,3] (reference layout, device), scale1/shift1 f32[16] folded BN of layer1.  out NHWC [B,H,W,16].
 */
int ppn_stem01(int32_t dtype, int32_t src_is_u8, const void* src, int32_t batch, int32_t h, int32_t w,
               const float* w0, const float* scale0, const float* shift0, const float* mean, const float* std_,
               const float* w1, const float* scale1, const float* shift1, void* out, void* stream);

/* A recorded sequence of launches (one forward pass): replayed in order on `stream`. */
typedef struct ppn_plan ppn_plan;
int ppn_plan_create(ppn_plan** out);
int ppn_plan_add_conv(ppn_plan* p, const ppn_conv_desc* d);
/* A whole 64-channel BasicBlock as one entry (ppn_basicblock64_fused). */
int ppn_plan_add_block(ppn_plan* p, const ppn_block_desc* d);
/* Zero `bytes` at `ptr` as a step of the plan (the arg-max keys of the fused head conv); runs as a KERNEL with
 * 16-byte stores, never a memset node of the captured graph: `ptr` must be 16-byte aligned (PPN_E_INVALID else). */
int ppn_plan_add_memset(ppn_plan* p, void* ptr, size_t bytes);
/* ppn_split_f16x3 as a step of the plan (PPN_F16X3 plans: behind the PPN_F32 launches whose outputs feed split convs). */
int ppn_plan_add_split(ppn_plan* p, const float* src, int64_t pixels, int32_t channels, void* dst);
int ppn_plan_add_stem(ppn_plan* p, int32_t dtype, int32_t src_is_u8, const void* src, int32_t batch, int32_t h,
                      int32_t w, const float* weight, const float* scale, const float* shift, const float* mean,
                      const float* std_, void* out);
int ppn_plan_add_stem01(ppn_plan* p, int32_t dtype, int32_t src_is_u8, const void* src, int32_t batch, int32_t h,
                        int32_t w, const float* w0, const float* scale0, const float* shift0, const float* mean,
                        const float* std_, const float* w1, const float* scale1, const float* shift1, void* out);
/* The whole stem in one launch, bf16 mode (csrc/stem012.hip): layer0 7x7 3->16, layer1 3x3 16->16, layer2 3x3 stride 2
 * 16->32, each + folded BN + ReLU (drn.py:123-133), input normalisation fused; out_raw = layer2's output, out_act =
 * relu(out_raw * scale3 + shift3), the pre-activation of the first BasicBlock (either may be NULL).  Outputs NHWC bf16
 * [B, (H+1)/2, (W+1)/2, 32].  Weights f32 in the reference layout; bit-identical to running ppn_stem7x7 +
 * two ppn_conv2d_fused launches in bf16 mode. */
int ppn_stem012(int32_t src_is_u8, const void* src, int32_t batch, int32_t h, int32_t w, const float* w0,
                const float* scale0, const float* shift0, const float* mean, const float* std_, const float* w1,
                const float* scale1, const float* shift1, const float* w2, const float* scale2, const float* shift2,
                const float* scale3, const float* shift3, void* out_raw, void* out_act, void* stream);
int ppn_plan_add_stem012(ppn_plan* p, int32_t src_is_u8, const void* src, int32_t batch, int32_t h, int32_t w,
                         const float* w0, const float* scale0, const float* shift0, const float* mean, const float* std_,
                         const float* w1, const float* scale1, const float* shift1, const float* w2, const float* scale2,
                         const float* shift2, const float* scale3, const float* shift3, void* out_raw, void* out_act);
/* The same with the 16-bit type as an argument: dtype = PPN_BF16 (== the two entry points above) or PPN_F16 (IEEE half
 * storage and MFMA operands, outputs NHWC f16). */
/* dtype of the *_dt entry points: PPN_BF16 / PPN_F16 = the stem's MFMA operand type, on-chip storage type and output
 * type; PPN_STEM_IO(PPN_F16, PPN_BF16) = IEEE-half operands and on-chip tensors, bf16 OUTPUT tensors (what the bf16 mode runs
 * since round 4: the stem's rounding noise is amplified by every layer behind it, csrc/stem012.hip). */
#define PPN_STEM_IO(internal, out) ((internal) | (((out) + 1) << 8))
/* PPN_STEM_IO(PPN_F16X3, PPN_F32): the stem for the exact modes (csrc/stem012_x3.hip) -- split-f16 internals with the error
 * model of a PPN_F16X3 convolution (activations and weights as half pairs hi = half(v), lo' = half((v - hi) * 2^11), weights
 * scaled by a power of two per layer, a_hi w_hi + a_hi w_lo + a_lo w_hi on f16 MFMAs with f32 accumulation, BN and ReLU in
 * f32; u8 frames keep the exact integer input), outputs NHWC f32 [B, (H+1)/2, (W+1)/2, 32] like the three PPN_F32
 * launches it replaces, within 1.2e-5 of the output scale of them.  Not combinable with PPN_STEM_RAW_S2; the layer-by-layer
 * entry points (ppn_stem7x7, ppn_stem01) reject it. */
/* PPN_STEM_RAW_S2 (or-ed into the dtype of the *_dt entry points; round 5): out_raw receives only the pixels with even row AND
 * column, as NHWC [batch, (Ho + 1) / 2, (Wo + 1) / 2, 32] -- when the raw stem output's only reader is the first BasicBlock's
 * 1x1 stride-2 projection (drn.py:53-54, 176-181), which reads exactly those pixels: 19 instead of 75 MB written at batch 32,
 * and the projection becomes a stride-1 launch over a dense tensor instead of a gather of half-used 128-byte lines. */
#define PPN_STEM_RAW_S2 (1 << 16)
int ppn_stem012_dt(int32_t dtype, int32_t src_is_u8, const void* src, int32_t batch, int32_t h, int32_t w, const float* w0,
                   const float* scale0, const float* shift0, const float* mean, const float* std_, const float* w1,
                   const float* scale1, const float* shift1, const float* w2, const float* scale2, const float* shift2,
                   const float* scale3, const float* shift3, void* out_raw, void* out_act, void* stream);
int ppn_plan_add_stem012_dt(ppn_plan* p, int32_t dtype, int32_t src_is_u8, const void* src, int32_t batch, int32_t h,
                            int32_t w, const float* w0, const float* scale0, const float* shift0, const float* mean,
                            const float* std_, const float* w1, const float* scale1, const float* shift1, const float* w2,
                            const float* scale2, const float* shift2, const float* scale3, const float* shift3,
                            void* out_raw, void* out_act);
/* Re-point the first layer's input (same shape/dtype as at ppn_plan_add_stem) before a run. */
int ppn_plan_set_input(ppn_plan* p, const void* src);
/* Issue every launch of the plan on `stream`.  After two launch-by-launch runs the sequence is captured into a
 * hipGraph per (input pointer, stream) and later runs are one hipGraphLaunch (PPN_PLAN_GRAPH=0 disables that; a
 * failed capture falls back to launch-by-launch -- the same kernels either way). */
int ppn_plan_run(ppn_plan* p, void* stream);
/* Same as ppn_plan_run but brackets every launch with HIP events on `stream`; ms[i] = duration of launch i.
 * Each launch is issued `repeats` (>= 1) times back to back between its two events and the elapsed time is
 * divided by `repeats`, which amortises the event/launch gap (launches are idempotent: no output aliases an
 * input).  Synchronises on the last event. */
int ppn_plan_run_timed(ppn_plan* p, void* stream, float* ms, int32_t n_ms, int32_t repeats);
/* Number of times the plan's launch sequence has been captured into a hipGraph (0 while it still launches directly).
 * A plan re-captures when its input pointer or its stream changes -- the old executable graph is retired only after
 * its stream has drained -- so callers that serve fresh frames keep ONE plan-owned input buffer per plan and copy
 * into it (PoseProposalNet._plan_for does); this counter lets tests assert that. */
int ppn_plan_graph_captures(const ppn_plan* p);
int ppn_plan_size(const ppn_plan* p);
/* Name of the kernel launch i dispatches (as it appears in rocprofv3 --kernel-trace). */
const char* ppn_plan_kernel_name(const ppn_plan* p, int32_t i);
int ppn_plan_destroy(ppn_plan* p);

/* Weight packing: reference layout f32 [cout,cin,k,k] -> [cout_pad][k_total] dtype, zero padded, with the
 * depth order/step reported by ppn_conv_tiling. */
int ppn_pack_weight(int32_t dtype, const float* w, int32_t cout, int32_t cin, int32_t ksize, int32_t cout_pad,
                    int32_t k_total, int32_t k_order, int32_t k_step, void* out, void* stream);
/* Same, for the input-gradient convolution of a layer whose FORWARD weight is w f32 [cin,cout,k,k]: packs
 * w'[co][ci][ky][kx] = w[ci][co][k-1-ky][k-1-kx] (cout/cin are those of the gradient convolution, i.e. the
 * forward layer's cin/cout).  ppn_conv2d_fused on dy with this weight is autograd's conv input gradient. */
int ppn_pack_weight_dgrad(int32_t dtype, const float* w, int32_t cout, int32_t cin, int32_t ksize, int32_t cout_pad,
                          int32_t k_total, int32_t k_order, int32_t k_step, void* out, void* stream);

/* All weight packs of a training iteration in ONE launch (round 4: a DRN-D-22 step packed its ~86 weight views -- each
 * layer's forward and input-gradient layout -- with one 8 us launch apiece, every optimiser step; the reference has no
 * counterpart: cuDNN reads its [cout,cin,k,k] parameters directly, /root/reference/main.py:643-777).
 * items (host): one entry per ppn_pack_weight / ppn_pack_weight_dgrad call it replaces, same arguments, same result.
 * ppn_pack_table_build lays the entries out for the device: `table` (host, n * PPN_PACK_ITEM_BYTES bytes) is what the
 * caller copies ONCE to device memory; total_blocks is the grid of ppn_pack_table_run, which re-packs every entry from
 * the current values of its w on `stream`.  Pointers are captured: rebuild the table when a w or out moves. */
typedef struct ppn_pack_item {
    const float* w;      /* device, reference layout f32 */
    void* out;           /* device, [cout_pad][k_total] of dtype (f32 for k_order 2) */
    int32_t dtype, cout, cin, ksize, cout_pad, k_total, k_order, k_step;
    int32_t transposed;  /* 1: ppn_pack_weight_dgrad's layout */
    int32_t reserved_;
} ppn_pack_item;
#define PPN_PACK_ITEM_BYTES 64
int ppn_pack_table_build(const ppn_pack_item* items, int32_t n, void* table, int32_t* total_blocks);
int ppn_pack_table_run(const void* table_dev, int32_t n, int32_t total_blocks, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training building blocks (main.py:623-777).  Activations are NHWC
 * [pixels][channels] in `dtype`, channels a multiple of 8 and a power of two <= 2048 (every BN of the
 * DRN-D / PPN stack); per-channel parameters, statistics and gradients are f32.
 * ---------------------------------------------------------------------------------------- */

/*
 * A16: nn.BatchNorm2d in train mode (implicit in model.train(), main.py:643) fused with the activation that
 * follows it (drn.py:44-51 ReLU, model.py:113-131 LeakyReLU(0.1)):
 *     mean_c, var_c  = batch statistics over all pixels (biased variance)
 *     y              = act((x - mean_c) / sqrt(var_c + eps) * gamma_c + beta_c)
 *     running_mean   = (1-momentum) * running_mean + momentum * mean_c
 *     running_var    = (1-momentum) * running_var  + momentum * var_c * n/(n-1)
 * save_mean / save_rstd [C] are kept for the backward; scale / shift [C] are the folded affine
 * (y = act(x*scale + shift)) a fused consumer can use instead of y.  y, running_*, scale, shift may be NULL.
 */
typedef struct ppn_bn_desc {
    int32_t dtype;
    int32_t channels;
    int64_t pixels;
    int32_t act;                  /* PPN_ACT_NONE / RELU / LRELU(0.1) */
    float eps, momentum;
    const void* x;
    const float* gamma;
    const float* beta;
    float* running_mean;
    float* running_var;
    float* save_mean;
    float* save_rstd;
    float* scale;
    float* shift;
    void* y;
    void* workspace;              /* >= ppn_bn_workspace_bytes(channels) */
    /* > 0: the workspace already holds that many blocks of partial sums { sum x, sum x^2 } per channel, written by the
     * convolution that produced x (ppn_conv_desc.stats_mode 1, *stats_tiles): the reduction pass over x is skipped. */
    int32_t stats_blocks;
    /* non-NULL (HOST int, needs y): the apply pass also folds { sum y, sum y^2 } of the values it stores into the workspace, as
     * the reduction pass of a BatchNorm over y would (bit for bit); *emit_blocks receives the number of partial blocks -- the
     * stats_blocks of that next call (same channel count, same workspace, nothing in between).  A pre-activation block's bn1
     * behind a conv-BN-ReLU unit (drn.py:47-63 after drn.py:205-218). */
    int32_t* emit_blocks;
} ppn_bn_desc;

size_t ppn_bn_workspace_bytes(int32_t channels);
int ppn_bn_train_fwd(const ppn_bn_desc* d, void* stream);

/*
 * Backward of the same fused BN + activation.  dy is the gradient w.r.t. y; with z = x_hat*gamma + beta,
 * g = dy * act'(z):   dgamma = sum g*x_hat,  dbeta = sum g,
 *                     dx = gamma*rstd * (g - dbeta/n - x_hat*dgamma/n)  (+ dx_add, e.g. the skip-path gradient)
 * dgamma / dbeta are OVERWRITTEN.  dx may alias dy or dx_add.
 */
typedef struct ppn_bn_bwd_desc {
    int32_t dtype;
    int32_t channels;
    int64_t pixels;
    int32_t act;
    const void* x;
    const void* dy;
    const void* dx_add;           /* NULL or [pixels][channels] */
    const float* gamma;
    const float* beta;
    const float* save_mean;
    const float* save_rstd;
    float* dgamma;
    float* dbeta;
    void* dx;
    void* workspace;              /* >= ppn_bn_workspace_bytes(channels) */
    /* > 0: the workspace already holds that many blocks of { sum g, sum g * xhat } per channel, written by the input-gradient
     * convolution that produced dy (ppn_conv_desc.stats_mode 2): the reduction pass over x and dy is skipped (single stream only). */
    int32_t stats_blocks;
    /* next_x non-NULL: the dx this call writes is the dy of ANOTHER BatchNorm (+ next_act) over next_x [pixels][channels] --
     * the projection shortcut's BatchNorm of the block below, or the conv-BN-ReLU unit below.  The apply pass folds that
     * BatchNorm's { sum g, sum g * xhat } from the dx it stores into the workspace (bit for bit what its reduction pass would
     * compute); *next_blocks (HOST int) receives the number of partial blocks = the stats_blocks of that next call. */
    const void* next_x;
    const float *next_gamma, *next_beta, *next_mean, *next_rstd;
    int32_t next_act;
    int32_t* next_blocks;
} ppn_bn_bwd_desc;

int ppn_bn_train_bwd(const ppn_bn_bwd_desc* d, void* stream);

/* out[c] = sum over pixels of x[p][c] (NHWC, channels a power of two in [8,2048]); the bias gradient of a
 * convolution whose output gradient is x (model.py:91 conv2.bias).  workspace >= ppn_bn_workspace_bytes(channels). */
int ppn_colsum(int32_t dtype, const void* x, int64_t pixels, int32_t channels, float* out, void* workspace,
               void* stream);

/*
 * Backward through the head's sigmoid (model.py:134) + relayout for the conv3 backward kernels:
 *     dz[b][hw][c] = grad_head[b][c][hw] * s*(1-s),  s = head[b][c][hw]          (NCHW f32 -> NHWC `dtype`)
 * Only the first channels_used (<= channels) channels of every image are converted (a probe pass of a unary loss
 * uses 6K of the 7605); dz has channels_pad (multiple of 64 >= channels_used) channels, the padding is zeros;
 * dbias (optional, f32[channels]) = sum over b,hw of the same quantity = d/d(conv3.bias).
 */
int ppn_head_grad(int32_t dtype, const float* head, const float* grad_head, int32_t batch, int32_t channels,
                  int32_t hw, int32_t channels_used, int32_t channels_pad, void* dz, float* dbias, void* stream);

/* Bottleneck tail (drn.py:92-95): out = relu(z + r), and its backward dz = dout * (out > 0) (+ add); n elements,
 * a multiple of 8, any contiguous layout. */
int ppn_add_relu(int32_t dtype, const void* z, const void* r, int64_t n, void* out, void* stream);
int ppn_relu_mask(int32_t dtype, const void* out, const void* dout, const void* add, int64_t n, void* dz, void* stream);

/* Data movement of the stride-2 input gradients and of the 7x7 layer's weight-gradient input in ONE pass each (torch did a
 * fill + a strided copy_, or four strided copies; main.py:677-683 leaves all of it to autograd / cuDNN):
 * ppn_upsample_zero:     dst [B][dst_h][dst_w][C] = src [B][src_h][src_w][C] at the pixels (y, x) = stride * (i, j), 0 elsewhere
 *                        (a pixel = a multiple of 16 bytes);
 * ppn_interleave_parity: dx [B][h][w][C] from the four parity sub-convolutions o_{py,px} [B][Ho+1][Wo+1][C] (Ho = (h+2-3)/2+1)
 *                        of a stride-2 3x3 input gradient: dx[y][x] = o_{y&1,x&1}[(y + (y&1)) / 2][(x + (x&1)) / 2];
 * ppn_image_to_nhwc:     f32 NCHW [B][3][h][w] -> NHWC [B][h][w][channels_pad] of dtype (channels_pad 4 or 8, channels 3.. zero). */
int ppn_upsample_zero(int32_t dtype, const void* src, int32_t batch, int32_t src_h, int32_t src_w, int32_t channels,
                      int32_t stride, int32_t dst_h, int32_t dst_w, void* dst, void* stream);
int ppn_interleave_parity(int32_t dtype, const void* o00, const void* o01, const void* o10, const void* o11, int32_t batch,
                          int32_t h, int32_t w, int32_t channels, void* dx, void* stream);
/* ppn_interleave_parity with the four sub-convolutions stacked along the channels of one tensor o [B][Ho+1][Wo+1][4 C]
 * (parity (py, px) in channel block 2 py + px): the output of ONE convolution with the four 2 x 2 filter sets stacked along
 * its output channels, which reads dy once instead of four times. */
int ppn_interleave_parity_stacked(int32_t dtype, const void* o, int32_t batch, int32_t h, int32_t w, int32_t channels, void* dx,
                                  void* stream);
int ppn_image_to_nhwc(int32_t dtype, const float* src, int32_t batch, int32_t h, int32_t w, int32_t channels_pad, void* dst,
                      void* stream);

/*
 * A15: one torch.optim.Adam step (main.py:278-279: betas (0.9, 0.999), eps 1e-8, weight_decay 0, no amsgrad)
 * over a flat f32 buffer -- the whole model is one launch.  `step` is the 1-based step count.
 *     m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g
 *     p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps)
 * grad_scale multiplies g first (1/world_size after the SUM all-reduce, main.py:1233-1238).
 * param_lp (optional) receives the updated parameters rounded to bf16 (the copy the bf16 kernels read).
 * Hyper-parameters are doubles (Python floats): torch forms 1-beta and the bias corrections in double.
 */
int ppn_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double lr,
                  double beta1, double beta2, double eps, double weight_decay, int32_t step, float grad_scale,
                  void* param_lp, void* stream);

/* sum of squares of a f32 buffer, written (not accumulated) to out[0]; deterministic.  n <= 2^31.
 * workspace >= 1024 doubles.  Building block of G_i = ||d(w_i L_i)/dW||_2 (main.py:704-717). */
int ppn_sumsq(const float* x, int64_t n, float* out, void* workspace, void* stream);

/*
 * The limb loss's probe gradient by linearity of the backward pass (the four unary probe gradients g_0..3 =
 * dL_i/dW of main.py:704-708 and total = sum_i c_i dL_i/dW from loss.backward(), main.py:677-683) and every norm
 * the GradNorm step needs of them, in ONE pass:
 *     gw4 = (total - sum_{i<4} c_i g_i) / c_4                      (f32[n] device, written)
 *     stats[0..3] = ||g_i||^2,  stats[4] = ||gw4||^2,  stats[5] = ||total - sum c_i g_i||^2,  stats[6] = ||total||^2
 * coeff: HOST pointer to 5 floats c_i, c_4 != 0.  Every sum equals ppn_sumsq of that tensor (same mapping and
 * reduction order; deterministic).  workspace >= 1024 * 7 doubles.
 */
int ppn_gradnorm_probe_stats(const float* g0, const float* g1, const float* g2, const float* g3, const float* total,
                             const float* coeff, int64_t n, float* gw4, float* stats, void* workspace, void* stream);

/*
 * A13: the task-weight half of the GradNorm step (main.py:717-765), all on device, one launch:
 *     l_i = w_i*L_i;  G_i = w_i*gnorm_i;  G_avg = mean G;  lhat_i = l_i/base_i;  r_i = lhat_i/mean(lhat)
 *     C_i = G_avg * r_i^alpha (constant);  Lgrad = sum |G_i - C_i|;  dLgrad/dw_i = sign(G_i - C_i)*gnorm_i
 *     Adam step on w (optimizerR)
 * gnorm_i = ||dL_i/dW||_2 for the probe weight W (head conv1.weight).  out5x4 (optional, f32[20]) receives
 * G, C, dw and [Lgrad, G_avg, 0, 0, 0] for logging / tests.
 */
int ppn_gradnorm_weight_step(float* w, const float* losses, const float* gnorm, const float* base, float alpha,
                             float* exp_avg, float* exp_avg_sq, double lr, double beta1, double beta2, double eps,
                             int32_t step, float* out5x4, void* stream);
/* main.py:767-777 after the all-reduce(SUM): w = clamp(w/world, min 0);  w /= mean(w). */
int ppn_gradnorm_renorm(float* w, int32_t world_size, void* stream);

/*
 * Convolution weight gradient (autograd of nn.Conv2d inside loss.backward(), main.py:677-683):
 *     dw[co][ci][ky][kx] = beta*dw + sum_{b,oy,ox} dy[b,oy,ox,co] * x[b, oy*stride+ky*dil-pad, ox*stride+kx*dil-pad, ci]
 * x, dy NHWC in `dtype` (cin, cout multiples of 8 for bf16 / 4 for f32), dw f32 in the REFERENCE layout
 * [cout,cin,k,k] (the layout of the flat gradient buffer the all-reduce and Adam work on).  Deterministic.
 * The input gradient needs no entry point of its own: it is ppn_conv2d_fused on dy with the weights transposed
 * and flipped (see pytorch_pose_proposal_network_amd/train.py: conv_dgrad).
 */
typedef struct ppn_wgrad_desc {
    int32_t dtype;
    int32_t batch, in_h, in_w, cin;
    int32_t out_h, out_w, cout;
    int32_t ksize, stride, dilation, pad;
    float beta;                   /* 0: overwrite dw, 1: accumulate into it */
    const void* x;
    const void* dy;
    float* dw;
    void* workspace;
    uint64_t workspace_bytes;     /* >= ppn_conv_wgrad_workspace_bytes(desc) */
} ppn_wgrad_desc;

/* The workspace holds one f32 partial [k*k][cout][cin] per pixel split.  bf16: a split covers at most 8 096 (>= 256-wide
 * layers) or 4 032 (narrower ones) output pixels -- its x-row offset table lives in LDS -- so the workspace grows with the
 * pixel count: 132 MB for a 512 -> 512 3x3 layer at 32 x 48 x 48 pixels (14 splits), ~75 splits per 600 k pixels. */
size_t ppn_conv_wgrad_workspace_bytes(const ppn_wgrad_desc* d);
int ppn_conv_wgrad(const ppn_wgrad_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Second-order pieces: GradNorm's Lgrad.backward() (main.py:759) differentiates the probe gradients
 * G_iR = d(w_i L_i)/dW (created with create_graph=True, main.py:704-708) once more.  With v_i = g_i/||g_i||,
 *     d||g_i||/dtheta = d/dtheta <grad_s L_i(s), sdot_i>,   sdot_i = forward-mode tangent of the head along the
 * weight direction v_i; only the head's tail (bn0_2 .. sigmoid) carries a tangent.  These entry points are the
 * non-linear building blocks of the reverse pass over that dual computation (the convolutions reuse
 * ppn_conv2d_fused / ppn_conv_wgrad on both streams).
 * ---------------------------------------------------------------------------------------- */

/* dst[b][hw][c] = src[b][c][hw] (f32 NCHW -> NHWC `dtype`, channels_pad a multiple of 64, padding zeroed). */
int ppn_nchw_to_nhwc(int32_t dtype, const float* src, int32_t batch, int32_t channels, int32_t hw,
                     int32_t channels_used, int32_t channels_pad, void* dst, void* stream);

/* dx = dy * act'(x*scale + shift) with the BN affine of (gamma, beta, save_mean, save_rstd): the activation mask of
 * a tangent that has passed the BN (its forward-mode image is ppn_bn_train_bwd with act NONE applied to the
 * tangent).  Uses x, dy, gamma, beta, save_mean, save_rstd, act, dx of the descriptor. */
int ppn_bn_act_mask(const ppn_bn_bwd_desc* d, void* stream);

/* Adjoint of the train-mode BN tangent  ydot = gamma*rstd*(xdot - mean(xdot) - xhat*mean(xhat*xdot))  followed by
 * the activation mask, with respect to x and gamma:  d->dy is the adjoint arriving at the masked tangent, `xdot`
 * the tangent that entered the BN.  d->dx is ACCUMULATED into (add it to the ordinary ppn_bn_train_bwd result);
 * dgamma_tan f32[C] is overwritten.  (The adjoint w.r.t. xdot itself is ppn_bn_train_bwd(x, dy, act).dx.)
 * d->workspace >= ppn_bn_dual_workspace_bytes(channels). */
size_t ppn_bn_dual_workspace_bytes(int32_t channels);
int ppn_bn_dual_bwd(const ppn_bn_bwd_desc* d, const void* xdot, float* dgamma_tan, void* stream);

/* The three calls above for `nstreams` gradient / tangent streams over the SAME x in one set of launches (round 4: the
 * second-order tail of the GradNorm step pushes five tangent streams -- one per loss, /root/reference/main.py:700-759 --
 * through two train-mode BNs; stream by stream that was ~160 launches of ~8 us per iteration).  Every per-pixel tensor
 * other than x (dy, dx, dx_add, xdot) holds the streams back to back: [nstreams][pixels][channels]; d->pixels is ONE
 * stream's pixel count; dgamma, dbeta, dgamma_tan are [nstreams][channels]; d->workspace >= nstreams *
 * ppn_bn_workspace_bytes (ppn_bn_dual_workspace_bytes for the dual call).  Stream s's results are bit-identical to the
 * single-stream call on its slices. */
int ppn_bn_train_bwd_streams(const ppn_bn_bwd_desc* d, int32_t nstreams, void* stream);
int ppn_bn_act_mask_streams(const ppn_bn_bwd_desc* d, int32_t nstreams, void* stream);
int ppn_bn_dual_bwd_streams(const ppn_bn_bwd_desc* d, const void* xdot, float* dgamma_tan, int32_t nstreams, void* stream);
/* ... with ONE d->dx [pixels][channels] that accumulates the term of every stream, in stream order (what the tail needs is
 * the adjoint at x summed over the streams: the ordinary backward is linear in dy, so its streams are summed BEFORE the
 * convolutions in front of it -- the primal adjoint chain of the second-order tail is a single stream). */
int ppn_bn_dual_bwd_streams_sum(const ppn_bn_bwd_desc* d, const void* xdot, float* dgamma_tan, int32_t nstreams,
                                void* stream);

/* Head-space seeds for one coefficient vector c (HOST, 5 floats): with s = head, sdot = s(1-s)*tz,
 *     tzbar = sdot_bar * sig'          sdot_bar = d(sum c_i L_i)/ds
 *     zbar  = s_bar*sig' + sdot_bar*sig''*tz,   s_bar = (d2(sum c_i L_i)/ds2) sdot   (dual-number evaluation)
 * all f32.  tz, zbar, tzbar have the head layout [B][C][H*W]; with unary_only != 0 they are compact tensors
 * [B][6K][H*W] holding only the unary channels (c[4] must be 0; weight_ij / te may be NULL). */
int ppn_loss_dual(const ppn_loss_cfg* cfg, const float* head, const float* tz, int32_t batch, const float* delta,
                  const float* weight, const float* weight_ij, const float* tx_half, const float* ty_half,
                  const float* tx, const float* ty, const float* tw, const float* th, const float* te,
                  const float* coeff, int32_t unary_only, float* zbar, float* tzbar, void* stream);

/*
 * The limb loss's stream of ppn_loss_dual -- coefficient vector (0, 0, 0, 0, c4) -- with the outputs in the layout the
 * convolutions read: zb, tzb `dtype` [B][H*W][cpad] NHWC (cpad a multiple of 64, >= 6K + E*sH*sW; channels outside the
 * limb range are zero) and zsum f32 [B][ceil(H*W/64)][cpad], the per-block pixel sums of zbar (summed over the first two
 * axes they are conv3.bias' second-order gradient).  Same arithmetic as ppn_loss_dual + ppn_nchw_to_nhwc without the two
 * f32 head-layout intermediates (2 x 17 MB per image written and re-read).
 */
int ppn_loss_limb_dual_nhwc(const ppn_loss_cfg* cfg, const float* head, const float* tz, int32_t batch,
                            const float* weight_ij, const float* te, float c4, int32_t dtype, int32_t cpad, void* zb,
                            void* tzb, float* zsum, void* stream);
int ppn_loss_limb_dual_nhwc_c(const ppn_loss_cfg* cfg, const float* head, const float* tz, int32_t batch,
                              const uint8_t* limb_compact, float c4, int32_t dtype, int32_t cpad, void* zb, void* tzb,
                              float* zsum, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PPN_H */
