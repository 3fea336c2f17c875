/*
 * nvq.h — C ABI of libnvq.so, the MI355X (gfx950) kernels behind
 * nerve_cl.models.SuperResolutionNet forward/backward and nerve_cl.continual.EWC.
 *
 * The reference (manikya7022/Continual-Learning-for-Dynamic-Video-Quality-Enhancement)
 * has no native / FFI boundary: its hot path is a chain of torch.nn calls.  Each entry
 * point below therefore names the reference torch call(s) it replaces (file:line,
 * relative to the reference checkout).  The Python host that binds these symbols is
 * nerve_cl/_nvq.py (ctypes); INTEGRATION.md shows the stub.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch caching allocator);
 *    the library never allocates, frees, synchronises or changes device: calls are
 *    stream-ordered on `stream` (a hipStream_t passed as void*) and graph-capturable.
 *  - activations are fp32 "NHWC with leading dimension": image n, pixel (y,x), channel c
 *    lives at base[((n*H + y)*W + x)*ld + coff + c].  A channel slice of a wider buffer
 *    (dense-block concat, frame-major aligned stack) is addressed by (base, ld, coff);
 *    ld and coff are in elements.  Tensors at the module boundary (frames in, SR frame
 *    out, parameters and their gradients) are fp32 NCHW / PyTorch layout.
 *  - return value: 0 on success, a negative NVQ_E* code otherwise; nvq_last_error()
 *    returns a thread-local description.  Nothing throws.
 */
#ifndef NVQ_H
#define NVQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NVQ_OK 0
#define NVQ_EINVAL (-1)   /* bad argument / unsupported shape */
#define NVQ_ELAUNCH (-2)  /* hipLaunch / hipGetLastError failure */
#define NVQ_EWORKSPACE (-3)

#define NVQ_MATH_F32 0    /* v_mfma_f32_16x16x4_f32: exact fp32 products and sums */
#define NVQ_MATH_BF16 1   /* operands rounded to bf16 in LDS, fp32 accumulate (v_mfma_f32_16x16x32_bf16) */

#define NVQ_MAX_T 8

int nvq_version(void);
const char* nvq_last_error(void);

/* ------------------------------------------------------------------ convolution
 * Dense k x k (k = 1 or 3), stride 1, zero "same" padding, cross-correlation
 * convention: replaces nn.Conv2d forward and, with a transposed pack, its input
 * gradient.  Reference call sites: flow_net super_resolution.py:74-82, attention
 * :168-175, ResidualDenseBlock :236-253, gff :308-311, upsampler conv
 * efficient_layers.py:94-100, pointwise :49-56. */

/* Packed-weight size in floats for a conv with `cout` outputs reading `cin_store`
 * stored input channels (cin_store % 4 == 0), for the given NVQ_MATH_* mode (the pack is
 * mode-specific: fp32 values in 16-channel chunks, or bf16 values in 32-channel chunks). */
size_t nvq_conv_pack_floats(int cout, int cin_store, int ksize, int math);

/* w: PyTorch layout [cout_w][cin_w][k][k].
 * transpose == 0: forward pack; output channels = cout_w, input channels = cin_w
 *                 (zero-padded up to cin_store).
 * transpose == 1: input-gradient pack; output channels = cin_w (only the first
 *                 `cout_keep` are kept), input channels = cout_w (padded to cin_store),
 *                 taps flipped. */
int nvq_conv_pack(const float* w, int cout_w, int cin_w, int ksize, int transpose,
                  int cin_store, int cout_keep, int math, float* wpack, void* stream);

/* Several nvq_conv_pack calls in one launch: a training step packs ~120 weights, and at small frame sizes every launch costs
 * ~18 us of device-side latency whatever its size.  Fields as the arguments of nvq_conv_pack; `jobs` is a host array. */
typedef struct nvq_pack_job {
    const float* w; int cout_w; int cin_w; int ksize; int transpose; int cin_store; int cout_keep; float* wpack;
} nvq_pack_job;
int nvq_conv_pack_batch(const nvq_pack_job* jobs, int njobs, int math, void* stream);

typedef struct nvq_conv_desc {
    const float* in;  int in_ld;  int in_coff;  int cin;       /* cin % 4 == 0 stored channels */
    const float* wpack;                                          /* from nvq_conv_pack */
    const float* bias;                                           /* [cout] or NULL */
    float* out;       int out_ld; int out_coff; int cout;      /* real output channels */
    int cout_store;                                              /* >= cout: channels [cout,cout_store) are written as the epilogue of a zero accumulator */
    float* out2;      int out2_ld; int out2_coff;               /* optional: value before residual/accumulate/mask */
    const float* res; int res_ld; int res_coff; int res_cmax;   /* residual added to out channels < res_cmax */
    const float* mask; int mask_ld; int mask_coff; int mask_c0; int mask_c1; /* out channels in [c0,c1) are zeroed where mask <= 0 */
    int n, h, w;
    int ksize;        /* 1 or 3 */
    int relu;         /* max(.,0) after bias */
    float alpha;      /* scale after relu */
    int accumulate;   /* out += result */
    int math;         /* NVQ_MATH_* */
    /* Storage type of each activation tensor: 0 = fp32, 1 = bf16 (ld / coff then count bf16 elements and the
     * pointer, although typed float*, addresses bf16 data).  bf16 tensors need NVQ_MATH_BF16, a bf16 input
     * needs cin, in_ld, in_coff % 8 == 0, and every slice must be 8-byte addressable. */
    int in_bf16, out_bf16, out2_bf16, res_bf16, mask_bf16;
    /* One-bit ReLU masks (NVQ_MATH_BF16, vector epilogue; cout <= 32, or a 3x3 conv of a bf16 input with more output channels):
     * word c / 32 of the bits_words (0 = 1) words of pixel (n*h + y)*w + x holds bit c % 32 = "output channel c of this pixel
     * is > 0".  bits_mode 1: written from the value stored to `out` (a conv + ReLU forward); bits_mode 2: read as the mask of
     * channels [0, cout_store) instead of a `mask` tensor (the input-gradient conv of the layer behind it: 4 bytes per pixel
     * and 32 channels instead of 64); 0: unused. */
    unsigned* bits;
    int bits_mode;
    /* 3x3 only, a hint: the packed weights of input channels [0, center_cin) are zero outside the centre tap (the
     * 0.2*lff^T part of the mirror-form dense-block gradient convs, nvq_rdb_backward_weights), so the kernel may skip the
     * other eight taps of those channels.  Multiple of 32, <= cin; 0 = no such channels.  Results do not depend on it. */
    int center_cin;
    /* Slice-planar input (NVQ_MATH_BF16, bf16 input, cin % 32 == 0, in_coff == 0): in_plane = elements of one 32-channel
     * plane = n*h*w*32.  The first in_ld channels (in_ld in {32, 64, 128}) are an ordinary [n][h][w][in_ld] tensor at `in`;
     * every further 32-channel chunk kc (>= in_ld/32) is a compact [n][h][w][32] tensor at in + kc*in_plane - the layout in
     * which a dense block's buffer is [x | y_0 | y_1 | ...] as separate tensors in one allocation, so that every 64-byte
     * pixel row a layer writes shares its 128-byte line with the next pixel, not with another layer.  0 = the usual
     * interleaved buffer.  Outputs, residuals and masks are ordinary (ld, coff) slices of those tensors in either case. */
    unsigned in_plane;
    /* Kernel-variant hint, results do not depend on it (beyond the fp32 summation order inside a 32-channel K chunk): 0 =
     * automatic; 8 = the 3x3 NVQ_MATH_BF16 kernels use their 8x32-pixel, four-wave form (the automatic choice for bf16 input is
     * an eight-wave form: 16x32 tiles for cout <= 32 - for images of fewer than 32 such tiles the 8x32 form -, two
     * 32-channel halves per workgroup for cout >= 64); for cout <= 32 also
     * 16 = the 16x32-tile kernel on v_mfma_f32_16x16x32_bf16, 162 / 164 = the same tile on v_mfma_f32_32x32x16_bf16 with two /
     * four tile rows per wave (automatic: 162 up to 128 input channels, 16 above); for cout >= 64 (a multiple of 64 stored channels,
     * bf16 output) 264 / 265 = v_mfma_f32_32x32x16_bf16 forms (a wave of 2 rows x 64 channels / eight channel-split waves;
     * measured slower or equal, never automatic).  Lets a caller A/B the forms without any
     * library state. */
    int tile_rows;
    /* words per pixel of `bits` (0 or 1: one word, cout <= 32) */
    int bits_words;
} nvq_conv_desc;
/* epilogue: v = acc + bias; if relu v = max(v,0); v *= alpha; out2 = v;
 *           if c < res_cmax v += res; if accumulate v += out; if mask<=0 on [c0,c1) v = 0; out = v */
int nvq_conv_forward(const nvq_conv_desc* d, void* stream);
/* Tail of ResidualDenseBlock.forward (super_resolution.py:245-253) in one launch: d3 = the last dense layer
 * (3x3, cin = F+128 -> 32 channels written in place at [cin, cin+32) of the bf16 concat buffer, bias + ReLU, optional
 * bits_mode 1), dl = the local feature fusion (1x1 over channels [0, cin+32) of the same buffer -> 64 channels, with
 * dl's alpha / res / out2 / output).  Same results as nvq_conv_forward(d3) followed by nvq_conv_forward(dl); the concat
 * buffer is read once instead of twice.  NVQ_MATH_BF16 only. */
int nvq_rdb_tail_forward(const nvq_conv_desc* d3, const nvq_conv_desc* dl, void* stream);
/* (The library keeps no mutable state: the diagnostic switches of tools/ - nvq_debug_* - exist only in the separate
 * libnvq_debug.so that `NVQ_DEBUG_TOOLS=1 build.sh` makes; tools/nvq_debug.h declares them.) */
size_t nvq_sizeof_conv_desc(void);

/* Combined weights for the backward of one ResidualDenseBlock (super_resolution.py:245-253) in "mirror"
 * form.  With the block's gradient buffer laid out [gout(F) | dy_4 | dy_3 | dy_2 | dy_1 | dy_0], the gradient
 * of growth slice y_i is ONE 3x3 convolution over the channel prefix [0, F+32(4-i)) (the 0.2*lff^T term on the
 * centre tap, the transposed/flipped dense-layer weights elsewhere), and the gradient w.r.t. the block input
 * is one more over all F+160 channels - no read-modify-write accumulation.
 * lff: [F][F+160][1][1]; w_i: [32][F+32i][3][3].  out holds, in PyTorch layout and in this order,
 * Wb_4 [32][F], Wb_3 [32][F+32], ..., Wb_0 [32][F+128], Wb_x [F][F+160]  (each [..][3][3]). */
size_t nvq_rdb_backward_weights_floats(int F);
int nvq_rdb_backward_weights(const float* lff, const float* w0, const float* w1, const float* w2,
                             const float* w3, const float* w4, int F, float* out, void* stream);

/* Weight (+ bias) gradient of the same convolution: replaces the parameter half of
 * aten::convolution_backward.  dw is PyTorch layout [cout][cin_w][k][k]; only the
 * first cin_w of the `cin` stored input channels receive a gradient.
 * dw = alpha * sum_pixels x (*) dy  (+ dw if accumulate), same for dbias. */
typedef struct nvq_wgrad_desc {
    const float* x;  int x_ld;  int x_coff;  int cin;  int cin_w;
    const float* dy; int dy_ld; int dy_coff; int cout;
    float* dw; float* dbias;            /* dbias may be NULL */
    float* workspace; size_t workspace_bytes;
    int n, h, w, ksize;
    float alpha; int accumulate; int math;
    int x_bf16, dy_bf16;                /* storage type of x / dy (see nvq_conv_desc); need NVQ_MATH_BF16 */
    unsigned x_plane;                   /* slice-planar x (see nvq_conv_desc::in_plane; bf16 x, x_coff == 0); 0 = interleaved */
    /* Kernel-variant hint, results do not depend on it (up to the summation order): 0 = automatic; 1 = always the
     * (pixel split, ci chunk, co chunk) kernels; 2 = always the all-input-channel kernels (an error for a shape they do not
     * take).  The all-input-channel kernels (bf16 x and dy; 3x3: cout = 32, slice-planar x, cin in {96, .., 192}; 1x1: cin in
     * {64, .., 256}, cout <= 64) read x without halo and dy once per launch, as persistent workgroups; automatic from four
     * 4x32-pixel tiles per workgroup on (smaller launches: the split kernels).  Lets a caller A/B the two forms.
     * 3 = as 1, and the split kernel keeps 32 output channels per workgroup where it would take 64 (3x3, bf16 x and dy,
     * cout > 32: eight waves stage the x tile once per 64 output channels). */
    int variant;
} nvq_wgrad_desc;
size_t nvq_wgrad_workspace_bytes(void);   /* upper bound valid for every shape */
int nvq_conv_wgrad(const nvq_wgrad_desc* d, void* stream);
/* The same in two halves, for steps that are bound by their launch count (the 64x64 continual-learning step): the weight-gradient
 * kernel alone leaves its partial sums in d->workspace and describes the reduce that finishes it in *job; nvq_wgrad_reduce_batch
 * runs up to 16 such reduces per launch (any n).  Every job needs a workspace of its own until its batch has run.  Results equal
 * nvq_conv_wgrad's bit for bit (same sums, same order). */
typedef struct {
    const float* part; const float* bias_part; float* dw; float* dbias;
    int nsplit, nci, nco, taps, cout, cin_w; float alpha; int accumulate;
} nvq_wgrad_reduce_job;
int nvq_conv_wgrad_partial(const nvq_wgrad_desc* d, nvq_wgrad_reduce_job* job, void* stream);
int nvq_wgrad_reduce_batch(const nvq_wgrad_reduce_job* jobs, int n, void* stream);
size_t nvq_sizeof_wgrad_desc(void);
size_t nvq_sizeof_wgrad_reduce_job(void);

/* Backward of  pointwise 1x1 conv (no bias) -> BatchNorm2d -> ReLU  of a DepthwiseSeparableConv (efficient_layers.py:49-66) in
 * the bf16 mode, 64 channels in and out: what nvq_bn_relu_backward + nvq_conv_forward (transposed pack) + nvq_conv_wgrad do
 * in three passes, after the BatchNorm sums in ONE pass over the tensors (dp = the BatchNorm-input gradient is formed in LDS
 * and never stored).  dy [N,H,W,dy_ld]: gradient w.r.t. relu(bn(p)), fp32 or bf16; p: the conv output = BatchNorm input, d: the
 * conv input (both bf16); groups of `group_images` images have their own statistics mean / invstd [G][64];
 * weight [64 co][64 ci] fp32.  Outputs: dd (bf16) = gradient w.r.t. d; dgamma, dbeta [64]; dweight [64][64] (all overwritten).
 * sums_in != NULL: the BatchNorm sums [G][2][64] already computed (nvq_dwconv_backward's bn_sums for the same dy and p):
 * the reduce pass is skipped and dgamma / dbeta are left alone (that call wrote them).
 * workspace: nvq_wgrad_workspace_bytes() is enough. */
int nvq_pw_bn_backward(const float* dy, int dy_ld, int dy_bf16, const float* p, int p_ld, const float* d, int d_ld,
                       int N, int group_images, int H, int W, const float* mean, const float* invstd,
                       const float* gamma, const float* beta, int training, const float* weight, float* dd, int dd_ld,
                       float* dgamma, float* dbeta, float* dweight, const float* sums_in, float* workspace,
                       size_t workspace_bytes, void* stream);
/* Flags bit of the _ex entry points below: the input gradient alone, without the weight gradient the full form forms as a side
 * product (a frozen layer).  The input gradient is bit-identical to the full form's; the weight-gradient outputs are neither
 * written nor read and may be NULL. */
#define NVQ_NO_WGRAD 2
/* "p is the output of nvq_dwpw_forward on this d and this weight" (nvq_pw_bn_backward_ex / _finish): the pass behind the
 * BatchNorm sums then forms p = bf16(d W^T) again from the d tile it stages anyway, bit for bit what is stored, instead of
 * reading it - one tensor pass fewer, every output bit-identical.  Honoured with a bf16 dy and without NVQ_NO_WGRAD; any
 * other call reads p as before.  The BatchNorm sums (sums_in == NULL) are still taken from the stored p. */
#define NVQ_PW_RECOMPUTE 4
/* nvq_pw_bn_backward with a flags word.  flags == 0: exactly nvq_pw_bn_backward.  NVQ_NO_WGRAD: dd alone - d is not read,
 * dweight is not written (may be NULL), no reduce launch.  dgamma / dbeta may be NULL (a frozen BatchNorm affine, with or without
 * the flag): the sums dd needs are still formed.  NVQ_PW_RECOMPUTE: see above. */
int nvq_pw_bn_backward_ex(const float* dy, int dy_ld, int dy_bf16, const float* p, int p_ld, const float* d, int d_ld,
                          int N, int group_images, int H, int W, const float* mean, const float* invstd,
                          const float* gamma, const float* beta, int training, const float* weight, float* dd, int dd_ld,
                          float* dgamma, float* dbeta, float* dweight, const float* sums_in, float* workspace,
                          size_t workspace_bytes, int flags, void* stream);

/* ------------------------------------------------------------------ feature extractor
 * FeatureExtractor.head, super_resolution.py:40-43: relu(conv3x3(frame; W[F,Cin,3,3], b)).
 * frames: fp32 NCHW clip (B,T,Cin,H,W) contiguous.  Output image index = slot*B + b
 * holds frame t = t_of_slot[slot]. */
int nvq_head_forward(const float* frames, int B, int T, int Cin, int H, int W,
                     const int* t_of_slot_host, int nslots,
                     const float* weight, const float* bias, int F,
                     float* out, int out_ld, int out_bf16, float* img8, int math, void* stream);
/* img8 (optional, bf16 [nslots*B][H][W][8]): the frames themselves in slot order, channels 0..Cin-1 (rest zero) - the
 * x operand with which nvq_conv_wgrad computes the head's weight gradient on the matrix cores in bf16 mode.
 * math: NVQ_MATH_F32 = exact fp32 FMAs; NVQ_MATH_BF16 = weights rounded to bf16, the frame taken as a hi + lo pair of bf16
 * values (~16 bits), fp32 accumulation on the matrix cores (Cin = 3, F in {16, 32, 64}; other shapes use the fp32 kernel
 * in either mode). */
/* dweight[F][Cin][3][3], dbias[F] (+= if accumulate) from (dout + dout2) masked by (act > 0); dout2 may be NULL
 * (it is the skip path of `features = body(h) + h`, summed here instead of in a separate pass). */
int nvq_head_wgrad(const float* frames, int B, int T, int Cin, int H, int W,
                   const int* t_of_slot_host, int nslots,
                   const float* dout, int dout_ld, const float* dout2, int dout2_ld,
                   const float* act, int act_ld, int F,
                   float* dweight, float* dbias, float* workspace, size_t workspace_bytes,
                   int accumulate, int act_bf16, void* stream);

/* Depthwise 3x3 (groups = C, no bias), efficient_layers.py:38-46.  weight [C][1][3][3].
 * flip == 1 gives the input gradient.  The *_bf16 flags of this section give the storage type of the
 * corresponding activation tensor (0 = fp32, 1 = bf16; arithmetic and statistics stay fp32). */
/* bn != NULL (bf16 input, C % 64 == 0): the kernel's input is relu(batchnorm(in)) evaluated on the fly with the given
 * per-(group, channel) statistics - the BatchNorm + ReLU of DepthwiseSeparableConv k feeding the depthwise conv of k+1
 * (efficient_layers.py:62-67) without a pass of its own.  mean/invstd: [N/group_images][C]; gamma/beta: [C]. */
typedef struct nvq_bn_input {
    const float* mean; const float* invstd; const float* gamma; const float* beta;
    int group_images;
} nvq_bn_input;
/* epi != NULL (same kernels): out = (conv + add) where mask > 0, else 0.  add: fp32 or bf16 (add_bf16) [.., add_ld] or NULL;
 * mask: fp32 or bf16 [.., mask_ld] or NULL.  Used for the last depthwise input gradient of the feature extractor, which so leaves the
 * kernel as the ReLU-masked gradient of the head conv (skip path added). */
typedef struct nvq_dw_epilogue {
    const float* add; int add_ld; const float* mask; int mask_ld; int mask_bf16; int add_bf16;
} nvq_dw_epilogue;
int nvq_dwconv_forward(const float* in, int in_ld, const float* weight, int C,
                       float* out, int out_ld, int N, int H, int W, int flip,
                       int in_bf16, int out_bf16, const nvq_bn_input* bn, const nvq_dw_epilogue* epi,
                       void* stream);
int nvq_dwconv_wgrad(const float* x, int x_ld, const float* dy, int dy_ld, int C,
                     int N, int H, int W, float* dweight, float* workspace,
                     size_t workspace_bytes, int accumulate, int x_bf16, int dy_bf16,
                     const nvq_bn_input* bn, void* stream);
/* Backward of the depthwise 3x3 conv of a DepthwiseSeparableConv (efficient_layers.py:49-66) in the bf16 mode, 64 channels:
 * what nvq_dwconv_wgrad + nvq_dwconv_forward(flip = 1) do in two launches, from one staged tile (x, dy -> dx; dy read once).
 * x [N,H,W,x_ld] bf16: the conv's input; bn != NULL: the input was relu(bn(x)) (evaluated while x is staged, as in
 * nvq_dwconv_wgrad); dy: gradient w.r.t. the conv output, bf16; weight [64][3][3] fp32.  Outputs: dx (bf16, overwritten) =
 * gradient w.r.t. the conv input, through the optional epilogue dx = (dx + add) where mask > 0 (add fp32, mask bf16);
 * dweight [64][3][3] (overwritten).  bn_sums != NULL (needs bn, no epi): the kernel holds both operands of the BACKWARD of that
 * BatchNorm + ReLU - its input x and the gradient dx of its output - and also returns the per-group sums bn_sums [G][2][64]
 * = {sum g, sum g xhat} (g = dx where relu(bn(x)) > 0) and bn_dgamma / bn_dbeta [64] (overwritten): what the first half of
 * nvq_bn_relu_backward / nvq_pw_bn_backward computes in a pass of its own; hand bn_sums to nvq_pw_bn_backward(sums_in).
 * workspace >= 512*(576+128) floats. */
int nvq_dwconv_backward(const float* x, int x_ld, const nvq_bn_input* bn, const float* dy, int dy_ld, const float* weight,
                        float* dx, int dx_ld, const nvq_dw_epilogue* epi, int N, int H, int W, float* dweight,
                        float* bn_sums, float* bn_dgamma, float* bn_dbeta, float* workspace, size_t workspace_bytes,
                        void* stream);
/* nvq_dwconv_backward with a flags word.  flags == 0: exactly nvq_dwconv_backward.  NVQ_NO_WGRAD: dx (and bn_sums) alone -
 * no depthwise weight gradient (dweight not written, may be NULL), x is staged only for bn_sums. */
int nvq_dwconv_backward_ex(const float* x, int x_ld, const nvq_bn_input* bn, const float* dy, int dy_ld, const float* weight,
                           float* dx, int dx_ld, const nvq_dw_epilogue* epi, int N, int H, int W, float* dweight,
                           float* bn_sums, float* bn_dgamma, float* bn_dbeta, float* workspace, size_t workspace_bytes,
                           int flags, void* stream);
/* Forward of  depthwise 3x3 -> pointwise 1x1 (no bias) -> BatchNorm2d statistics  of a DepthwiseSeparableConv
 * (efficient_layers.py:49-66) in the bf16 mode, 64 channels: what nvq_dwconv_forward + nvq_conv_forward (1x1) + nvq_bn_stats
 * do in three launches (five tensor passes), in one pass x -> d, p.  in [N,H,W,in_ld] bf16; bn != NULL: x := relu(bn(x)) is
 * applied while the halo is staged (the previous layer's BatchNorm + ReLU, as in nvq_dwconv_forward; its group_images must be
 * `group_images`); dw_weight [64][3][3], pw_weight [64 co][64 ci] fp32.  Outputs (bf16, overwritten): d = the depthwise
 * result (the backward's operand), p = the pointwise result = BatchNorm input.  stats != 0: the batch statistics of p (of
 * the stored bf16 values) per group of `group_images` images go to mean / invstd [G][64] and are folded into running_mean /
 * running_var (either may be NULL) in the order order_host[0..G-1] (host array; NULL: 0..G-1), exactly as nvq_bn_stats does; workspace >= 512*128 floats.
 * stats == 0: p and d only (eval mode: the caller takes mean / invstd from nvq_bn_eval_stats). */
int nvq_dwpw_forward(const float* in, int in_ld, const nvq_bn_input* bn, const float* dw_weight, const float* pw_weight,
                     float* d, int d_ld, float* p, int p_ld, int N, int group_images, int H, int W, int stats, float eps,
                     float momentum, const int* order_host, float* mean, float* invstd, float* running_mean, float* running_var,
                     float* workspace, size_t workspace_bytes, void* stream);

/* BatchNorm2d, efficient_layers.py:59,65.  The N images form G = N/group_images groups
 * (one per feature-extractor call); statistics are per (group, channel) over
 * group_images*H*W pixels.
 * nvq_bn_stats: training statistics.  mean/invstd: [G][C] (saved for backward).
 *   running_* are updated once per group in the order order_host[0..G-1] (the reference
 *   calls the extractor for t = 0..T-1, super_resolution.py:347-349): momentum 0.1,
 *   unbiased variance.  running_* may be NULL. */
int nvq_bn_stats(const float* x, int x_ld, int C, int N, int group_images, int H, int W,
                 float eps, float momentum, const int* order_host,
                 float* mean, float* invstd, float* running_mean, float* running_var,
                 float* workspace, size_t workspace_bytes, int x_bf16, void* stream);
/* Evaluation: fill mean/invstd [G][C] from the running statistics. */
int nvq_bn_eval_stats(const float* running_mean, const float* running_var, int C, int G,
                      float eps, float* mean, float* invstd, void* stream);
/* y = relu(gamma*(x-mean)*invstd + beta) (+ res).  Images [0, split_images) go to outA,
 * the rest to outB (image index rebased): lets the centre frame land directly in its
 * slot of the frame-major aligned stack (super_resolution.py:352,357). */
int nvq_bn_apply_relu(const float* x, int x_ld, int C, int N, int group_images, int H, int W,
                      const float* mean, const float* invstd, const float* gamma,
                      const float* beta, const float* res, int res_ld,
                      float* outA, int outA_ld, int outA_coff, int split_images,
                      float* outB, int outB_ld, int outB_coff, int x_bf16, int out_bf16, int res_bf16,
                      void* stream);
/* Backward of y = relu(bn(x)).  dy is the gradient w.r.t. y; the ReLU mask is recomputed
 * from x and the statistics (gamma*(x-mean)*invstd + beta > 0), so y itself is not needed.
 * training != 0: batch-statistics backward; else running-statistics backward.
 * dgamma/dbeta [C]: summed over all groups, (+)= if accumulate. */
int nvq_bn_relu_backward(const float* dy, int dy_ld, const float* x, int x_ld, int C, int N,
                         int group_images, int H, int W, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, int training,
                         float* dx, int dx_ld, float* dgamma, float* dbeta,
                         float* workspace, size_t workspace_bytes, int accumulate,
                         int dy_bf16, int x_bf16, int dx_bf16, void* stream);

/* ------------------------------------------------------------------ motion
 * LiteFlowNetCorrelation(d=4).forward, efficient_layers.py:313-343.
 * out[n,p, i*9+j] = (1/C) sum_c x1[n,p,c] * x2[n, p + (i-4, j-4), c]; channels 81..out_ld-1
 * of each pixel are written as zero.  x2 image index = n % x2_images (centre-frame
 * features are shared by the T-1 reference frames).
 * math == NVQ_MATH_BF16 (and C in {32, 64}): the products run on the bf16 matrix cores (x1 / x2 rounded to bf16,
 * fp32 accumulation), out may be stored as bf16 (out_bf16; out_ld then a multiple of 8) and x1 / x2 may be bf16-stored
 * feature tensors (in_bf16, both; their ld then count bf16 elements and are multiples of 8).  Otherwise exact fp32. */
int nvq_correlation_forward(const float* x1, int x1_ld, const float* x2, int x2_ld,
                            int x2_images, int C, int N, int H, int W,
                            float* out, int out_ld, int math, int out_bf16, int in_bf16, void* stream);
/* which == 1: dx[n,p,c] (+)= (1/C) sum_d dcorr[n,p,d] * other[n % other_images, p+off(d), c]
 *             (gradient w.r.t. x1; other = x2)
 * which == 2: dx[n,q,c] (+)= (1/C) sum_d dcorr[n,q-off(d),d] * other[n, q-off(d), c]
 *             (gradient w.r.t. x2 contributed by image n; other = x1, other_images = N).
 *             groups > 1: dcorr and other hold groups * N images (frame-major: the T - 1 reference frames of every clip);
 *             dx[n] collects from images n, n + N, ... in that order in ONE pass (one read-modify-write of the shared
 *             centre-frame gradient instead of one per frame)
 * math / dcorr_bf16 / other_bf16 as above; the bf16 path reads dcorr up to channel 96 (dcorr_ld >= 96).  dx is fp32.
 * dx_bf16_out != NULL (matrix-core path): this is the LAST pass over an accumulated gradient - the result (dx + the new
 * term when accumulate) is written as bf16 to dx_bf16_out [N,H,W,dx_bf16_ld] channels [0,C) instead of back to dx, which
 * is only read: the readers of the finished gradient then move half the bytes.  addends (optional, with dx_bf16_out): up to
 * two more terms of that gradient, bf16 tensors [N,H,W,ld] read at channels [coff, coff + C), added in the same pass (with
 * accumulate == 0, dx is not touched at all - the whole sum is formed here, no fp32 accumulator, no separate add kernel). */
typedef struct nvq_corr_addends {
    const void* a; int a_ld; int a_coff;
    const void* b; int b_ld; int b_coff;
} nvq_corr_addends;
int nvq_correlation_backward(int which, const float* dcorr, int dcorr_ld,
                             const float* other, int other_ld, int other_images, int C, int N,
                             int H, int W, float* dx, int dx_ld, int dx_coff, int accumulate,
                             int math, int dcorr_bf16, int other_bf16, int groups, float* dx_bf16_out, int dx_bf16_ld,
                             const nvq_corr_addends* addends, void* stream);

/* warp_features, super_resolution.py:104-143 (F.grid_sample bilinear, zeros,
 * align_corners=True at pixel coordinates (x+flow_x, y+flow_y)). flow: [N,H,W,flow_ld>=2] fp32.
 * feat_bf16 / out_bf16: storage type of the two feature tensors (fp32 interpolation arithmetic either way). */
int nvq_warp_forward(const float* feat, int feat_ld, const float* flow, int flow_ld,
                     int C, int N, int H, int W, float* out, int out_ld, int out_coff,
                     int feat_bf16, int out_bf16, void* stream);
/* overwrite == 0: dfeat must be pre-initialised (the gradient is ADDED to it); overwrite != 0 (gather form only, 16 more
 * bytes of records): dfeat [N,H,W,0..C) is WRITTEN - no zero fill before and no read-modify-write in the call.  dflow
 * [N,H,W,dflow_ld] gets channels 0,1 written and 2..dflow_ld-1 zeroed.  records == NULL: scatter form, 4 float atomics per (pixel, channel).  records != NULL (20 bytes
 * per pixel of scratch, 16-byte aligned): gather form - a per-source pass writes the flow gradient and a {corner offset,
 * 4 weights} record, a per-destination pass collects the contributions from the 9x9 window around each pixel; no atomics
 * and a fixed summation order for every source whose flow is shorter than 4 pixels (longer ones are still scattered).
 * feat_bf16 / dout_bf16: `feat` (read for the flow gradient) / `dout` are stored as bf16 - gather form only; dfeat and
 * dflow are fp32 - except dfeat in the overwrite mode with dfeat_bf16 != 0: the gather pass then writes bf16 (the far sources
 * and the hit-list overflow add with a compare-and-swap loop per 32-bit word). */
int nvq_warp_backward(const float* dout, int dout_ld, int dout_coff, const float* feat,
                      int feat_ld, const float* flow, int flow_ld, int C, int N, int H, int W,
                      float* dfeat, int dfeat_ld, float* dflow, int dflow_ld,
                      float* records, size_t records_bytes, int feat_bf16, int dout_bf16, int overwrite, int dfeat_bf16,
                      void* stream);
/* nvq_warp_backward with a flags word.  flags == 0: exactly nvq_warp_backward (workspace unused).
 * NVQ_WARP_DETERMINISTIC (gather form in the overwrite mode only; anything else is NVQ_EINVAL): no float atomics - the
 * sources that move 4 px or more are binned by destination tile and gathered, so that every element of dfeat is one fp32
 * sum (window sources in scan order, then those far sources in ascending source-pixel index, then the window sources past
 * the per-pixel list, in scan order) stored once: bit-identical from run to run and independent of the other images of the
 * batch; a bf16 dfeat is rounded once.  dflow is bit-identical to nvq_warp_backward's.  workspace: device memory of
 * nvq_warp_backward_workspace_bytes(N, H, W, flags) = 4 * (3 * tiles + 9 * N*H*W) bytes with tiles =
 * N * ceil(H/8) * ceil(W/32) (0 without the flag), 4-byte aligned, no initialisation needed; sized for every source being
 * far, no host synchronisation (graph-capturable).  N*H*W < 2^29, H and W < 32767. */
#define NVQ_WARP_DETERMINISTIC 1
size_t nvq_warp_backward_workspace_bytes(int N, int H, int W, int flags);
int nvq_warp_backward_ex(const float* dout, int dout_ld, int dout_coff, const float* feat,
                         int feat_ld, const float* flow, int flow_ld, int C, int N, int H, int W,
                         float* dfeat, int dfeat_ld, float* dflow, int dflow_ld,
                         float* records, size_t records_bytes, int feat_bf16, int dout_bf16, int overwrite,
                         int dfeat_bf16, int flags, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ temporal aggregation
 * TemporalAggregator.forward softmax + weighted sum, super_resolution.py:174,203-204:
 * attn = softmax_t(logits[n,p,0..T-1]); weighted[n,p,c] = sum_t aligned[n,p,t*C+c]*attn_t.
 * Also emits per-block channel sums of `weighted` for the CBAM global average pool:
 * gap_partial [N][nblk][C] with nblk = nvq_tsum_blocks(H,W). */
int nvq_tsum_blocks(int H, int W);
int nvq_tsum_forward(const float* aligned, int aligned_ld, const float* logits, int logits_ld,
                     int T, int C, int N, int H, int W, float* attn, int attn_ld,
                     float* weighted, int weighted_ld, float* gap_partial, int aligned_bf16, int weighted_bf16,
                     void* stream);
/* aligned_bf16 (here and below): `aligned` is stored as bf16 (aligned_ld counts bf16 elements).  weighted_bf16 /
 * dweighted_bf16 / x_bf16 (here and in the CBAM calls below): the aggregated feature tensor `weighted` (= the CBAM's x), the
 * gradient that enters the CBAM backward (dout) and the one that leaves it (dx = dweighted) are stored as bf16 - the bf16
 * activation mode of the network; the pooled sums (gap_partial, sm, dca_partial) are formed from unrounded values either way. */
/* dw = dweighted + dgap_pix[n][c] (dgap_pix may be NULL);
 * daligned[n,p,t*C+c] = dw*attn_t ; dlogits = softmax backward of sum_c dw*aligned_t. */
int nvq_tsum_backward(const float* dweighted, int dweighted_ld, const float* dgap_pix,
                      const float* aligned, int aligned_ld, const float* attn, int attn_ld,
                      int T, int C, int N, int H, int W, float* daligned, int daligned_ld,
                      float* dlogits, int dlogits_ld, int aligned_bf16, int daligned_bf16, int dweighted_bf16,
                      void* stream);

/* CBAM, efficient_layers.py:154-228.
 * cbam_channel: gap = mean(weighted); hid = relu(W1 gap); ca = sigmoid(W2 hid).
 *   w1 [R][C], w2 [C][R]; outputs gap [N][C], hid [N][R], ca [N][C]. */
int nvq_cbam_channel(const float* gap_partial, int nblk, int C, int R, int N, int HW,
                     const float* w1, const float* w2, float* gap, float* hid, float* ca,
                     void* stream);
/* sm[n,p,0] = mean_c(x*ca), sm[n,p,1] = max_c(x*ca); amax = argmax channel. sm ld = 2. */
int nvq_cbam_pool(const float* x, int x_ld, const float* ca, int C, int N, int H, int W,
                  float* sm, int* amax, int x_bf16, void* stream);
/* sa = sigmoid(conv7x7(sm; w[1][2][7][7], pad 3)); out = x*ca*sa written at (out,ld,coff); out_bf16 != 0
 * stores bf16 (the destination is the first dense block's concat buffer). */
int nvq_cbam_spatial_apply(const float* x, int x_ld, const float* ca, const float* sm,
                           const float* w7, int C, int N, int H, int W, float* sa,
                           float* out, int out_ld, int out_coff, int out_bf16, int x_bf16, void* stream);
/* Backward through out = x*ca*sa:
 * step1: dpre[n,p] = (sum_c dout*x*ca) * sa*(1-sa)                                   */
int nvq_cbam_bwd_spatial_pre(const float* dout, int dout_ld, int dout_coff, const float* x,
                             int x_ld, const float* ca, const float* sa, int C, int N,
                             int H, int W, float* dpre, int x_bf16, void* stream);
/* step2: dsm = conv7x7^T(dpre) [N,H,W,2]; dw7[1][2][7][7] (+)= sum sm (*) dpre */
int nvq_cbam_bwd_spatial_conv(const float* dpre, const float* sm, const float* w7, int N,
                              int H, int W, float* dsm, float* dw7, float* workspace,
                              size_t workspace_bytes, int accumulate, void* stream);
/* flags == 0: exactly nvq_cbam_bwd_spatial_conv.  NVQ_NO_WGRAD: dsm alone (sm not read, dw7 not written, no workspace). */
int nvq_cbam_bwd_spatial_conv_ex(const float* dpre, const float* sm, const float* w7, int N,
                                 int H, int W, float* dsm, float* dw7, float* workspace,
                                 size_t workspace_bytes, int accumulate, int flags, void* stream);
/* step3: dxc = dout*sa + dsm0/C + [c==amax] dsm1 ; dx = dxc*ca ;
 *        dca_partial[n][blk][c] = block sums of dxc*x   (nblk = nvq_tsum_blocks) */
int nvq_cbam_bwd_scale(const float* dout, int dout_ld, int dout_coff, const float* x, int x_ld,
                       const float* ca, const float* sa, const float* dsm, const int* amax,
                       int C, int N, int H, int W, float* dx, int dx_ld, float* dca_partial,
                       int x_bf16, void* stream);
/* step4: through sigmoid / FC / relu / FC / mean: dw1, dw2 (+)=; dgap_pix[n][c] = dgap/HW */
int nvq_cbam_bwd_channel(const float* dca_partial, int nblk, int C, int R, int N, int HW,
                         const float* w1, const float* w2, const float* gap, const float* hid,
                         const float* ca, float* dw1, float* dw2, float* dgap_pix,
                         int accumulate, void* stream);
/* flags == 0: exactly nvq_cbam_bwd_channel.  NVQ_NO_WGRAD: dgap_pix alone (dw1 / dw2 not written, may be NULL). */
int nvq_cbam_bwd_channel_ex(const float* dca_partial, int nblk, int C, int R, int N, int HW,
                            const float* w1, const float* w2, const float* gap, const float* hid,
                            const float* ca, float* dw1, float* dw2, float* dgap_pix,
                            int accumulate, int flags, void* stream);

/* The whole upsampler tail in one launch (NVQ_MATH_BF16, bf16 input): PixelShuffleUpsampler.conv (3x3, cin -> Cimg*s*s, bias;
 * efficient_layers.py:94-100) whose epilogue puts the tile's conv outputs through LDS, reads them back as s x s pixel blocks
 * (PixelShuffle, :101-106), adds the bicubic skip of frames[:, t_center] and clamps (super_resolution.py:378-382): the
 * conv output never exists as a tensor.  d: in / wpack / bias / cin / cout = Cimg*s*s / n, h, w (output fields unused);
 * out, pass as nvq_shuffle_bicubic_clamp below, to which (after nvq_conv_forward) the result is bit-identical.  s in {2, 3, 4}. */
int nvq_upsampler_tail_forward(const nvq_conv_desc* d, const float* frames, int T, int t_center, int Cimg, int s,
                               float* out, uint8_t* pass, void* stream);

/* ------------------------------------------------------------------ upsampler tail
 * PixelShuffle(s) + bicubic skip + clamp, efficient_layers.py:101-106 and
 * super_resolution.py:378-382: out[b,c,h*s+i,w*s+j] =
 *   clamp(u[b,h,w,c*s*s+i*s+j] + bicubic(frames[b,t_center])[b,c,h*s+i,w*s+j], 0, 1).
 * out: fp32 NCHW (B,Cimg,H*s,W*s); pass: uint8 1 where 0 <= pre-clamp <= 1. */
int nvq_shuffle_bicubic_clamp(const float* u, int u_ld, const float* frames, int B, int T,
                              int t_center, int Cimg, int H, int W, int s, float* out,
                              uint8_t* pass, void* stream);
/* EnhancementEngine strength blend, enhancement_engine.py:172-180:
 * out = strength * sr + (1 - strength) * F.interpolate(frames[:, t_center], bicubic, align_corners=False).
 * sr / out: fp32 NCHW (B,Cimg,H*s,W*s); frames: fp32 (B,T,Cimg,H,W). */
int nvq_bicubic_blend(const float* sr, const float* frames, int B, int T, int t_center, int Cimg,
                      int H, int W, int s, float strength, float* out, void* stream);
/* du[b,h,w,c*s*s+i*s+j] = dout[b,c,h*s+i,w*s+j] * pass ; channels up to u_ld zero-filled */
int nvq_shuffle_clamp_backward(const float* dout, const uint8_t* pass, int B, int Cimg, int H,
                               int W, int s, float* du, int du_ld, void* stream);

/* ------------------------------------------------------------------ input gradients (frames)
 * Input gradient of FeatureExtractor.head / LightweightSuperResolution net.0 (3x3 conv, F -> Cin, Cin in {1, 3}):
 * dframes[b, t, ci, y, x] (+= if accumulate) = sum_{f,ky,kx} g[slot*B+b, y+1-ky, x+1-kx, f] * weight[f, ci, ky, kx],
 * frame t = t_of_slot[slot], dframes fp32 (B,T,Cin,H,W) contiguous.  g: dout as given when act == NULL (the pre-masked
 * gradient of the bf16 path), else (dout + dout2) where act > 0 (dout2 may be NULL), the operands nvq_head_wgrad takes.
 * dout / act: fp32 or bf16 (*_bf16) NHWC [nslots*B][H][W][ld], dout2 fp32; ld % 8 == 0, 16-B aligned; F % 16 == 0, <= 256.
 * Every output element is summed by one thread in a fixed order (no atomics): bit-reproducible. */
int nvq_head_dgrad(const float* dout, int dout_ld, int dout_bf16, const float* dout2, int dout2_ld,
                   const float* act, int act_ld, int act_bf16, const float* weight, int F,
                   int B, int T, int Cin, int H, int W, const int* t_of_slot_host, int nslots,
                   float* dframes, int accumulate, void* stream);
/* Adjoint of the bicubic skip (F.interpolate(frames[:, t_center], scale_factor=s, bicubic, align_corners=False)):
 * dframes[b, t_center, c] (+= if accumulate) = coef * B^T (dout * pass); dout fp32 (B,Cimg,H*s,W*s), pass uint8 of the same
 * layout or NULL (no mask), dframes fp32 (B,T,Cimg,H,W).  Gather form, every LR pixel summed by one thread in a fixed
 * order, clamped border taps included (no atomics).  s in 1..4. */
int nvq_bicubic_adjoint(const float* dout, const uint8_t* pass, int B, int Cimg, int H, int W, int s,
                        int T, int t_center, float coef, float* dframes, int accumulate, void* stream);
/* nvq_head_dgrad's pre-masked form for a gradient laid out by slot in either dimension: slot s reads images
 * s*slot_images + b (slot_images = B: time-major batch [nslots*B][H][W][ld]; 0: one image per b, [B][H][W][ld]) at
 * channels coff_of_slot[s] .. + F (a multiple of 8, + F <= ld).  FrameRecoveryNet's first temporal conv in the
 * time-in-channels layout: frame t at channel offset t*Cp.  Same kernel as nvq_head_dgrad (bit-identical results for
 * slot_images = B, offsets 0). */
int nvq_head_dgrad_tc(const float* dout, int dout_ld, int dout_bf16, const float* weight, int F,
                      int B, int T, int Cin, int H, int W, const int* t_of_slot_host,
                      const int* coff_of_slot_host, int nslots, int slot_images, float* dframes,
                      int accumulate, void* stream);
/* Input gradient of FrameRecoveryNet's stem nn.Conv2d(4, Co, 7, 2, 3, bias=False) on x4 = [frame | mask] (NHWC):
 * dx = stem^T(dy); channels 0..2 go to dframe (N,3,H,W) fp32 NCHW, channel 3 to dmask (N,1,H,W); either may be NULL (not
 * both); += if accumulate.  dy fp32 or bf16 (dy_bf16) [N][OH][OW][dy_ld], OH = (H-1)/2+1, dy_ld % 8 == 0, 16-B aligned;
 * w [Co,4,7,7]; Co in {16, 32, 48, 64}.  Gather form, fixed sum order (no atomics): bit-reproducible. */
int nvq_stem7_dgrad(const float* dy, int dy_ld, int dy_bf16, const float* w, int N, int H, int W, int Co,
                    float* dframe, float* dmask, int accumulate, void* stream);
/* FrameRecoveryNet blend backward with its inputs' gradients: drec as nvq_mask_blend_backward (ld rec_ld, channels
 * [C, ld) zeroed), dframe (N,C,H,W) = dout*(1-m), dmask (N,1,H,W) = sum_c dout*(rec-frame) (overwrite); dframe / dmask
 * may be NULL, frame and rec are read only for dmask. */
int nvq_mask_blend_backward_ex(const float* dout, const float* frame, const float* rec, int rec_ld,
                               const float* mask, int N, int C, int H, int W, float* drec,
                               float* dframe, float* dmask, void* stream);

/* nn.PixelShuffle(s) alone (stand-alone PixelShuffleUpsampler, efficient_layers.py:101-106):
 * img[b,c,h*s+i,w*s+j] = u[b,h,w,c*s*s+i*s+j] (backward != 0: the other direction, padding channels of u zeroed) */
int nvq_pixel_shuffle(float* u, int u_ld, int B, int C, int H, int W, int s, float* img, int backward,
                      void* stream);

/* ------------------------------------------------------------------ loss
 * nn.MSELoss() of the training loops (experiments/train_baseline.py:64,86, train_continual.py:31,55) and F.mse_loss of
 * EWC.compute_fisher (ewc.py:125): *out = mean((a - b)^2) over n floats; workspace >= 8 KiB. */
int nvq_mse_forward(const float* a, const float* b, long n, float* out, float* workspace,
                    size_t workspace_bytes, void* stream);
/* da = (*grad_out_dev) * 2 (a - b) / n  (grad_out_dev: device scalar, NULL for 1) */
int nvq_mse_backward(const float* a, const float* b, long n, const float* grad_out_dev, float* da,
                     void* stream);

/* ------------------------------------------------------------------ quality metrics and losses (csrc/quality.hip)
 * x = prediction, y = target: contiguous fp32, 16-byte aligned.  No float atomics: every entry point is deterministic. */
#define NVQ_LOSS_L1 0          /* |x - y|;                  slope sign(x - y), sign(0) = 0 */
#define NVQ_LOSS_CHARBONNIER 1 /* sqrt((x - y)^2 + eps^2);  slope (x - y) / sqrt((x - y)^2 + eps^2) */
#define NVQ_LOSS_MSE 2         /* (x - y)^2;                slope 2 (x - y) */
/* One pass over both tensors.  out (double [B][8], device): per sample n, sum x, sum y, sum x^2, sum y^2, sum xy,
 * sum |x - y|, sum (x - y)^2 over its `per` elements.  workspace >= B * min(1024, ceil(per / 4096)) * 28 bytes. */
int nvq_quality_sums(const float* x, const float* y, int B, long per, double* out, float* workspace,
                     size_t workspace_bytes, void* stream);
/* out[g] = mean over group g's `per` elements of the NVQ_LOSS_* `kind` (groups = 1: the whole tensor; groups = B: one
 * value per sample).  eps: Charbonnier only.  workspace >= groups * 8 KiB. */
int nvq_pixel_loss_forward(const float* x, const float* y, int groups, long per, int kind, float eps, float* out,
                           float* workspace, size_t workspace_bytes, void* stream);
/* dx = grad_out_dev[g] * slope(x - y) / per  (grad_out_dev: `groups` device floats, NULL for 1) */
int nvq_pixel_loss_backward(const float* x, const float* y, int groups, long per, int kind, float eps,
                            const float* grad_out_dev, float* dx, void* stream);
/* Windowed SSIM of [B][C][H][W] planes, H, W >= 11: per channel an 11 x 11 Gaussian window (sigma 1.5, separable, taps
 * normalised in fp32), valid positions only, biased local statistics, C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2;
 * the map is averaged over the valid positions and channels of a sample (per_sample != 0: out[B]) or of the whole batch
 * (out[1]); as_loss != 0 writes 1 - that mean.  Neither the map nor any moment reaches memory.
 * workspace >= B * C * ceil((H - 10) / 32) * ceil((W - 10) / 64) * 4 bytes. */
int nvq_ssim_forward(const float* x, const float* y, int B, int C, int H, int W, float data_range, int per_sample,
                     int as_loss, float* out, float* workspace, size_t workspace_bytes, void* stream);
/* dx = scale * grad_out_dev[b] * d(mean SSIM of sample b) / dx  (grad_per_sample != 0: B device floats), or
 * dx = scale * grad_out_dev[0] * d(mean SSIM of the batch) / dx  (grad_per_sample == 0); NULL grad_out_dev reads as 1.
 * Recomputes the moments per tile (nothing is saved by the forward); gather form, fixed tap order. */
int nvq_ssim_backward(const float* x, const float* y, int B, int C, int H, int W, float data_range,
                      const float* grad_out_dev, int grad_per_sample, float scale, float* dx, void* stream);
/* Multi-scale SSIM (Wang, Simoncelli, Bovik 2003) of `planes` = B * C planes of H x W over `scales` <= 8 scales, scale j
 * (0-based) being (H >> j) x (W >> j): x_0 = x, x_{j+1} = 2 x 2 mean of x_j.  With the window and constants of nvq_ssim_*,
 * m_j(plane) = mean over the valid positions of cs = (2 s_xy + C2) / (s_xx + s_yy + C2) for j < scales - 1 and of the SSIM map
 * for the last scale; v(plane) = prod_j max(m_j, 0)^weights[j]; ms(b) = mean over b's channels of v.  The coarsest scale must
 * hold a window: min(H, W) >> (scales - 1) >= 11.  The caller owns the pyramid; every call is one launch, deterministic.
 * The local moments are taken about 0.5 * data_range (variances do not depend on the centre; E[x^2] - mu^2 then does not
 * cancel), so a coarse scale of a few positions is as accurate as the mean over a full-size plane.
 * px, py [planes][H / 2][W / 2] = 2 x 2 mean, stride 2, of x, y [planes][H][W] (H, W >= 2; an odd last row or column is
 * dropped), summed in avg_pool2d's order. */
int nvq_avgpool2_pair(const float* x, const float* y, int planes, int H, int W, float* px, float* py, void* stream);
/* Bytes of the forward's workspace (one float per tile of every scale); 0 for arguments out of range. */
size_t nvq_msssim_workspace_bytes(int planes, int H, int W, int scales);
/* Tile sums of scale `scale` (xs, ys: that scale's planes; H, W: the finest scale's size) into its part of the workspace.
 * workspace >= nvq_msssim_workspace_bytes(planes, H, W, scales); all scales of one forward share it. */
int nvq_msssim_scale_forward(const float* xs, const float* ys, int planes, int H, int W, int scales, int scale,
                             float data_range, float* workspace, size_t workspace_bytes, void* stream);
/* After every scale's forward: out[b] = ms(b) (per_sample != 0: B floats) or out[0] = mean_b ms(b); as_loss != 0 writes 1 - that.
 * mtable [scales][B * C] = m_j, dtable [scales][B * C] = d ms(b) / d m_j(b, c), 0 where m_j <= 0 (a clamped term has value 0 and
 * gradient 0, never 0 * inf).  weights: `scales` positive device floats.  Sums and powers in double, fixed order. */
int nvq_msssim_finalize(const float* workspace, int B, int C, int H, int W, int scales, const float* weights, int per_sample,
                        int as_loss, float* out, float* mtable, float* dtable, void* stream);
/* dx [B * C][H >> scale][W >> scale] = sign * grad_out_dev[b] * d ms(b) / d xs (grad_per_sample != 0: B device floats), or
 * sign * grad_out_dev[0] * d(mean_b ms(b)) / d xs; NULL grad_out_dev reads as 1.  Only this scale's own term m_`scale` is
 * differentiated here; dx_coarser (NULL, or the gradient with respect to scale + 1's planes) enters through the pooling
 * adjoint: dx[r][c] += 0.25 dx_coarser[r / 2][c / 2] where that element exists.  Called from the coarsest scale to the finest,
 * the last call leaves the whole gradient.  No workspace. */
int nvq_msssim_scale_backward(const float* xs, const float* ys, int B, int C, int H, int W, int scales, int scale,
                              float data_range, const float* dtable, const float* grad_out_dev, int grad_per_sample,
                              float sign, const float* dx_coarser, float* dx, void* stream);

/* ------------------------------------------------------------------ distillation losses (csrc/distill.hip)
 * s = student, t = teacher, y = target: contiguous fp32, 16-byte aligned; the gradient is with respect to s only.  No float
 * atomics: every entry point is deterministic. */
/* One pass over s, t and y (y may be NULL: its term is 0).  Per group g of `per` elements (groups = 1: the whole tensor;
 * groups = B: one per sample) d = mean (s - t)^2 and m = mean (s - y)^2; out [3][groups] = wt d + wy m, d, m.
 * workspace >= groups * 16 KiB. */
int nvq_distill_forward(const float* s, const float* t, const float* y, int groups, long per, float wt, float wy, float* out,
                        float* workspace, size_t workspace_bytes, void* stream);
/* ds = grad_out_dev[g] * (2 / per) * (wt (s - t) + wy (s - y))  (grad_out_dev: `groups` device floats, NULL for 1); one
 * launch, ds written once */
int nvq_distill_backward(const float* s, const float* t, const float* y, int groups, long per, float wt, float wy,
                         const float* grad_out_dev, float* ds, void* stream);
/* Cosine distance of [B][C][hw] feature tensors over the channels of every position p: a = sum_c s^2, b = sum_c t^2,
 * ab = sum_c s t, v_p = 1 - ab / (max(sqrt a, eps) max(sqrt b, eps)).  out[b] = mean of v_p over sample b's positions
 * (per_sample != 0: B floats) or out[0] = the mean over all B * hw positions.  workspace >= B * 4 KiB. */
int nvq_cosine_distill_forward(const float* s, const float* t, int B, int C, int hw, float eps, int per_sample, float* out,
                               float* workspace, size_t workspace_bytes, void* stream);
/* ds_c = -(grad_out_dev[b or 0] / N) * (t_c / (ns nt) - [sqrt a > eps] cos_p s_c / a), N = hw (per_sample != 0) or B * hw;
 * NULL grad_out_dev reads as 1.  The moments are recomputed (two sweeps over C); no workspace. */
int nvq_cosine_distill_backward(const float* s, const float* t, int B, int C, int hw, float eps, const float* grad_out_dev,
                                int per_sample, float* ds, void* stream);

/* ------------------------------------------------------------------ FrameRecoveryNet layers (csrc/fr_ops.hip)
 * Generic NHWC kernels for reference nerve_cl/models/frame_recovery.py:23-446 (+ efficient_layers.py:109-151,
 * 231-294).  Tensors are [N,H,W,ld], logical channel count C <= ld, ld % 4 == 0, channels [C, ld) kept 0; fp32, or -
 * where an entry point has a `bf16` flag and it is set - bf16 for every activation tensor of that call (statistics,
 * parameters and their gradients are always fp32). */
/* dst[n,p,dst_coff+c] = src[n*src_nstride + c*H*W + p] (c < C), 0 for C <= c < czero: NCHW image (or frame t of a
 * (B,T,C,H,W) clip: src + t*C*H*W, src_nstride = T*C*H*W) into an NHWC slice */
int nvq_nchw_to_nhwc(const float* src, long src_nstride, int N, int C, int H, int W, float* dst,
                     int dst_ld, int dst_coff, int czero, void* stream);
int nvq_nhwc_to_nchw(const float* src, int src_ld, int src_coff, int N, int C, int H, int W,
                     float* dst, long dst_nstride, void* stream);
/* nn.BatchNorm2d / BatchNorm3d (frame_recovery.py:45,73,285-305; efficient_layers.py:139,266,279) for any C: statistics
 * over all npix pixels (train: batch mean / biased variance, running statistics updated with the unbiased variance;
 * running_mean may be NULL), then y = bn(x) (+ res) (ReLU if relu).  workspace >= nvq_bn2_workspace_bytes(C)
 * (+ 2*C floats for the backward). */
size_t nvq_bn2_workspace_bytes(int C);
int nvq_bn2_stats(const float* x, int x_ld, int C, long npix, float eps, float momentum, float* mean,
                  float* invstd, float* running_mean, float* running_var, float* workspace,
                  size_t workspace_bytes, int bf16, void* stream);
int nvq_bn2_eval_stats(const float* running_mean, const float* running_var, int C, float eps,
                       float* mean, float* invstd, void* stream);
int nvq_bn2_apply(const float* x, int x_ld, int C, long npix, const float* mean, const float* invstd,
                  const float* gamma, const float* beta, const float* res, int res_ld, int relu,
                  float* out, int out_ld, int bf16, void* stream);
/* g = dy masked by the forward ReLU (recomputed from x, res); dgamma = sum g*xhat, dbeta = sum g; dx as BatchNorm's
 * backward (training) or gamma*invstd*g (eval); dres = g when res != NULL */
int nvq_bn2_backward(const float* dy, int dy_ld, const float* x, int x_ld, int C, long npix,
                     const float* mean, const float* invstd, const float* gamma, const float* beta,
                     const float* res, int res_ld, int relu, int training, float* dx, int dx_ld,
                     float* dres, int dres_ld, float* dgamma, float* dbeta, float* workspace,
                     size_t workspace_bytes, int bf16, void* stream);
/* nvq_bn2_backward with a flags word.  flags == 0: exactly nvq_bn2_backward, except that dgamma and / or dbeta may be NULL
 * (a frozen BatchNorm affine: that store is dropped; in training mode the reduction still runs, dx needs its sums).
 * NVQ_NO_WGRAD: neither dgamma nor dbeta is written (both may be NULL).  In eval mode (training == 0) with no affine gradient,
 * dx and dres take one element-wise pass: no reduction and no workspace (may be NULL).  dx and dres are bit-identical to the
 * full form's. */
int nvq_bn2_backward_ex(const float* dy, int dy_ld, const float* x, int x_ld, int C, long npix,
                        const float* mean, const float* invstd, const float* gamma, const float* beta,
                        const float* res, int res_ld, int relu, int training, float* dx, int dx_ld,
                        float* dres, int dres_ld, float* dgamma, float* dbeta, float* workspace,
                        size_t workspace_bytes, int bf16, int flags, void* stream);
/* nn.MaxPool2d(k, s, pad) (frame_recovery.py:46) and F.max_pool3d(x, (1,2,2)) (:155,158): first maximum in scan order
 * wins (PyTorch's tie rule, matters after ReLU); idx = one byte per element; the backward is a gather (no atomics) */
int nvq_maxpool_forward(const float* x, int ld, int N, int H, int W, int k, int s, int pad, float* out,
                        uint8_t* idx, int bf16, void* stream);
int nvq_maxpool_backward(const float* dy, const uint8_t* idx, int ld, int N, int H, int W, int k, int s,
                         int pad, float* dx, int bf16, void* stream);
/* input side of nn.Conv2d(k=1, stride=2) (frame_recovery.py:71): out[n,y,x] = in[n,2y,2x]; backward = zero insertion
 * (in = gradient at the subsampled size, out = gradient at H x W) */
int nvq_subsample2(const float* in, int ld, int N, int H, int W, float* out, int backward, int bf16, void* stream);
/* F.interpolate(mode='bilinear', align_corners=False) (frame_recovery.py:224-229,433-436); backward (gather form):
 * in = dy [N,OH,OW], out = dx [N,H,W] */
int nvq_bilinear_resize(const float* in, int ld, int N, int H, int W, int OH, int OW, float* out,
                        int backward, void* stream);
/* nn.ConvTranspose2d(k=4, s=2, p=1) (frame_recovery.py:283-304) = 3x3 conv to 4*Co phase-major channels followed by
 * depth-to-space: nvq_convt_pack builds the [4*Co, Ci, 3, 3] conv weight from [Ci, Co, 4, 4], nvq_convt_unpack_grad
 * maps its gradient back, nvq_depth_space2 moves [N,H,W,4*Co] <-> [N,2H,2W,Co] */
int nvq_convt_pack(const float* w, int Ci, int Co, float* w3, void* stream);
int nvq_convt_unpack_grad(const float* dw3, int Ci, int Co, float* dw, void* stream);
int nvq_depth_space2(const float* in, float* out, int N, int H, int W, int Co, int to_depth, int bf16, void* stream);
/* TemporalConv3D's nn.Conv3d(Ci, Co, (3,1,1)) weight [Co,Ci,3,1,1] (efficient_layers.py:271-278) -> three 1x1 conv
 * weights [3][Co][Ci] (to_taps = 1) and back (its gradient, to_taps = 0): the temporal conv runs as three accumulating
 * 1x1 convolutions over time-shifted image ranges */
int nvq_tconv_relayout(const float* in, float* out, int Co, int Ci, int to_taps, void* stream);
/* The same convolution over a time-in-channels activation [B,H,W,T*Cp] (frame t = channels [t*Cp, t*Cp + C)): frame t of the
 * output is ONE 1x1 convolution over the channels of frames t-1..t+1 with the taps side by side - no accumulating passes.
 * nvq_tconv_cat lays taps k0 .. k0+nk-1 out as [Co][nk*Cp] (transpose = 0: forward / weight-gradient form) or as
 * [Ci][nk*Cp] with the tap order reversed (transpose = 1: input-gradient form over dy frames); padding columns are 0.
 * nvq_tconv_grad_combine folds the gradients of the first-frame (taps 1,2), middle (taps 0..2, may be NULL) and last-frame
 * (taps 0,1) forms back into dw [Co,Ci,3,1,1]. */
int nvq_tconv_cat(const float* w, int Co, int Ci, int Cp, int k0, int nk, int transpose, float* out, void* stream);
int nvq_tconv_grad_combine(const float* g_first, const float* g_mid, const float* g_last, int Co, int Ci, int Cp,
                           float* dw, void* stream);
/* per-image partial channel sums [N][nvq_gap_blocks(H,W)][C]: the input of nvq_cbam_channel for a stand-alone CBAM */
int nvq_gap_blocks(int H, int W);
int nvq_gap_partial(const float* x, int ld, int C, int N, int H, int W, float* part, void* stream);
/* x[n,p,c] += v[n,c] (gradient of the global average pool) */
int nvq_add_image_channel(float* x, int ld, int C, int N, int H, int W, const float* v, void* stream);
/* nn.Tanh (frame_recovery.py:309): out = tanh(a) | backward: out = a * (1 - y^2) */
int nvq_tanh(const float* a, const float* y, long n, float* out, int backward, void* stream);
/* FusionModule (frame_recovery.py:239-254): out = aligned + a0*mean_c(sp) + a1*mean_c(tp), (a0,a1) = softmax(logits[0:2]);
 * attn / means: [npix][2] saved for the backward; C a power of two in [16,256]; aligned / out / dy have ld = C */
int nvq_fusion_mix_forward(const float* aligned, const float* logits, int logits_ld, const float* sp,
                           int sp_ld, const float* tp, int tp_ld, int C, long npix, float* out,
                           float* attn, float* means, void* stream);
int nvq_fusion_mix_backward(const float* dy, const float* attn, const float* means, int C, long npix,
                            float* dlogits, int logits_ld, float* dsp, int sp_ld, float* dtp, int tp_ld,
                            void* stream);
/* FrameRecoveryNet blend (frame_recovery.py:439-440): out = frame*(1-m) + rec*m; frame/out NCHW, rec NHWC, m [N,1,H,W] */
int nvq_mask_blend(const float* frame, const float* rec, int rec_ld, const float* mask, int N, int C,
                   int H, int W, float* out, void* stream);
int nvq_mask_blend_backward(const float* dout, const float* mask, int N, int C, int H, int W,
                            float* drec, int rec_ld, void* stream);
/* SpatialEncoder stem nn.Conv2d(4, Co, 7, 2, 3, bias=False) (frame_recovery.py:42-44) on a 4-channel NHWC image;
 * w / dw in PyTorch layout [Co,4,7,7]; wgrad workspace >= 256*64*196 floats */
int nvq_stem7_forward(const float* x, const float* w, int N, int H, int W, int Co, float* out, int out_ld,
                      int out_bf16, void* stream);
int nvq_stem7_wgrad(const float* x, const float* dy, int dy_ld, int N, int H, int W, int Co, float* dw,
                    float* workspace, size_t workspace_bytes, int dy_bf16, void* stream);
/* dst[p, dst_coff + c] (+)= alpha * src[p, src_coff + c], c < C, each side fp32 or bf16 ([npix, ld] tensors): storage-type
 * boundary of FrameRecoveryNet's bf16 stages, mean / broadcast over the time groups (frame_recovery.py:164-165) */
int nvq_cast_slice(float* dst, int dst_ld, int dst_coff, int dst_bf16, const float* src, int src_ld,
                   int src_coff, int src_bf16, int C, long npix, float alpha, int accumulate, void* stream);

/* ------------------------------------------------------------------ small helpers */
/* dst[n,p,dst_coff+c] (+)= alpha*src[n,p,src_coff+c] [* (mask[n,p,mask_coff+c] > 0)] for c < C; src may be stored as
 * bf16 (src_bf16), dst and mask are fp32 */
int nvq_axpy_slice(float* dst, int dst_ld, int dst_coff, const float* src, int src_ld,
                   int src_coff, const float* mask, int mask_ld, int mask_coff, int C,
                   long npix, float alpha, int accumulate, int src_bf16, void* stream);
/* out[c] (+)= alpha * sum_pixels x[p, coff + c] */
int nvq_colsum(const float* x, int x_ld, int x_coff, int C, long npix, float alpha,
               float* out, float* workspace, size_t workspace_bytes, int accumulate,
               void* stream);

/* ------------------------------------------------------------------ return_intermediate tensors (csrc/intermediates.hip)
 * SuperResolutionNet.forward(return_intermediate=True), super_resolution.py:384-389: the `features`, `aligned` and
 * `aggregated` tensors live in the engine as NHWC channel slices (fp32 or bf16); at the module boundary they are fp32 NCHW
 * [N,C,H,W] tensors of the autograd graph.  Every job of one launch has the same N, C, H, W; C a power of two in [16, 256];
 * a slice needs a 16-B aligned base and ld, coff multiples of 4 (fp32) or 8 (bf16).  Any H, W; njobs <= NVQ_LAYOUT_MAX_JOBS. */
#define NVQ_LAYOUT_MAX_JOBS (2 * NVQ_MAX_T + 1)
#define NVQ_INJECT_MAX_SRC 4
typedef struct {
    const void* src; int src_ld, src_coff, src_bf16;   /* NHWC slice: fp32, or bf16 when src_bf16 */
    float* dst;                                        /* fp32 NCHW */
} nvq_gather_job;
typedef struct {
    void* dst; int dst_ld, dst_coff, dst_bf16;         /* NHWC gradient slice: fp32, or bf16 when dst_bf16 */
    const float* src[NVQ_INJECT_MAX_SRC];              /* fp32 NCHW upstream gradients; NULL entries are skipped */
} nvq_inject_job;
/* Forward: dst[n,c,y,x] = (float)src[n,y,x,coff+c] for every job: a widening copy, bit-exact. */
int nvq_gather_nchw(const nvq_gather_job* jobs, int njobs, int N, int C, int H, int W, void* stream);
/* Backward: dst[n,y,x,coff+c] = ((dst + src[0]) + src[1]) + ... in fp32 (that order, NULL sources skipped), a bf16 dst
 * rounded once (RNE).  No atomics: deterministic.  A job's dst must not be one of its sources. */
int nvq_inject_nchw(const nvq_inject_job* jobs, int njobs, int N, int C, int H, int W, void* stream);
size_t nvq_sizeof_gather_job(void);
size_t nvq_sizeof_inject_job(void);

/* ------------------------------------------------------------------ EWC (flat buckets)
 * EWC.penalty, ewc.py:195-232: penalty = lambda/2 * sum F*(theta-theta_star)^2 over a flat
 * bucket of n floats; result written to *out (device scalar). */
int nvq_ewc_penalty(const float* theta, const float* theta_star, const float* fisher,
                    long n, float lambda, float* out, float* workspace,
                    size_t workspace_bytes, void* stream);
/* grad (+)= (*scale_dev) * lambda * F * (theta - theta_star): gradient of the penalty
 * times the upstream scalar gradient (device pointer, may be NULL for 1). */
int nvq_ewc_penalty_grad(const float* theta, const float* theta_star, const float* fisher,
                         long n, float lambda, const float* scale_dev, float* grad,
                         int accumulate, void* stream);
/* EWC.compute_fisher accumulation, ewc.py:139-141: fisher += grad^2 */
int nvq_fisher_accumulate(const float* grad, long n, float* fisher, void* stream);
/* SynapticIntelligence on flat buckets (theta, grad, p_old, W, omega in one layout, n floats each).
 * update_importance, ewc.py:343-354:  W += -grad * (theta - p_old);  p_old = theta.
 * register_task, ewc.py:356-368:      omega += W / ((theta - p_old)^2 + damping);  W = 0;  p_old = theta.
 * (The penalty si_lambda * sum omega (theta - p_old)^2, ewc.py:370-379, is nvq_ewc_penalty with lambda = 2 si_lambda.) */
int nvq_si_update(const float* theta, const float* grad, long n, float* p_old, float* W, void* stream);
int nvq_si_consolidate(const float* theta, long n, float damping, float* p_old, float* W, float* omega, void* stream);

/* ------------------------------------------------------------------ gradient projection and clipping (csrc/bucket_ops.hip)
 * A-GEM (Chaudhry et al. 2019) and global-norm clipping on flat fp32 gradient buckets, without a host read.  `acc` is a
 * caller-owned device buffer of 5 doubles: acc[0] = g.r, acc[1] = r.r, acc[2] = g.g, acc[3] = projection coefficient c,
 * acc[4] = number of projections so far (the caller zeroes it once).
 *
 * nvq_bucket_moments: one pass over g and r (n floats each, 4-byte aligned): exact products, sums in double, per-block
 * partials in the workspace (>= 24 KiB, 8-byte aligned) and one finishing block; no atomics, the grid depends on n only, so
 * the sums are bit-reproducible and do not depend on the alignment of g / r.  acc[0..2] = the sums, or += with `accumulate`
 * (several segments chained into one acc).  r == NULL: g.g only (acc[0], acc[1] are zeroed, or kept with `accumulate`).
 * `coefficient` (the last segment's call): then c = acc[0] / acc[1] when acc[0] < 0 and acc[1] > 0, else 0 (a NaN compares
 * false); acc[4] += 1 when c != 0. */
int nvq_bucket_moments(const float* g, const float* r, long n, double* acc, int accumulate, int coefficient,
                       float* workspace, size_t workspace_bytes, void* stream);
/* g[i] = fmaf(-(float)c, r[i], g[i]) with c = acc[3] read on the device; c == 0 leaves g untouched (bit-identical) */
int nvq_bucket_project(float* g, const float* r, long n, const double* acc, void* stream);
/* torch.nn.utils.clip_grad_norm_ (2-norm) from acc[2] = g.g over all segments: coef = max_norm / (sqrt(acc[2]) + 1e-6);
 * g[i] *= coef only when coef < 1, otherwise g is untouched.  *norm_out (device, may be NULL) = the total norm. */
int nvq_bucket_clip(float* g, long n, const double* acc, float max_norm, float* norm_out, void* stream);

/* ------------------------------------------------------------------ Adam / AdamW on flat buffers (csrc/optim.hip)
 * torch.optim.Adam / AdamW (amsgrad = False, maximize = False) over n floats of theta, grad, exp_avg (m), exp_avg_sq (v) and,
 * when ema != NULL, an exponential moving average of theta, in one launch.  Per element, every operation rounded once:
 *   clip      acc != NULL (the 5 doubles of nvq_bucket_moments): coef = max_norm / (sqrt(acc[2]) + 1e-6);
 *             g = grad * (float)coef only when coef < 1 (a NaN compares false: unscaled), as nvq_bucket_clip decides; else g = grad.
 *             grad itself is never written.
 *   decay     decoupled (AdamW): theta *= (float)(1 - lr * weight_decay);  else (L2): g = fma(weight_decay, theta, g)
 *   moments   m = fma(g - m, one_minus_beta1, m);  v = fma(one_minus_beta2 * g, g, beta2 * v)
 *   update    theta = fma(-(float)(lr / bias1), m / (sqrt(v) / bias2_sqrt + eps), theta)
 *   ema       ema = fma(theta - ema, (float)(1 - ema_decay), ema)      [= ema_decay * ema + (1 - ema_decay) * theta]
 * bias1 = 1 - beta1^t, bias2_sqrt = sqrt(1 - beta2^t), one_minus_beta1 = 1 - beta1 and one_minus_beta2 = 1 - beta2 are formed by
 * the caller in double from the integer step count t and the betas and passed rounded to float, as torch's scalars are (1 - beta2
 * formed from a float beta2 would be off by 2^-16 relative at beta2 = 0.999).
 * The pointers need 4-byte alignment only: float4 accesses when all of them are 16-byte aligned, else four scalar accesses of the
 * same quads - the same bits either way.  The grid depends on n only; no atomics, no workspace.  n == 0 succeeds without a
 * launch.  Zeros in theta, grad, m, v and ema (bucket padding) stay exactly zero. */
int nvq_adam_step(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, long n, float lr, float beta1,
                  float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay, int decoupled,
                  float bias1, float bias2_sqrt, float ema_decay, const double* acc, float max_norm, void* stream);

/* ------------------------------------------------------------------ device-resident episodic memory (csrc/replay.hip)
 * The memory is a set of caller-owned tables with `capacity` rows (capacity <= 65536): lr_store [capacity][lr_per] and
 * hr_store [capacity][hr_per] (fp32, or bf16 when store_bf16), means [capacity][channels] fp32 (per-channel mean of the LR
 * sample), importance fp32, time int32 (store counter), access_count int32, type_id int32 (< 0: the slot is empty).
 * Slot indices come from device memory; a kernel skips an index outside [0, capacity).  No atomics, no workspace. */
#define NVQ_REPLAY_MEANS_ONLY 1   /* nvq_replay_store flag: write only means[slots[j]] (the other tables may be NULL) */
/* Sample j of src_lr [n][lr_per] / src_hr [n][hr_per] (fp32) goes to row slots[j] (distinct); bf16 storage rounds to
 * nearest even (NaN -> 0x7fc0, subnormals kept).  Also: importance / time / type_id [slot] = sample_* [j], access_count
 * [slot] = 0, and means[slot][c] = mean of LR plane c (second launch; double sums in a fixed order: reproducible bits). */
int nvq_replay_store(const float* src_lr, const float* src_hr, int n, long lr_per, long hr_per, int channels,
                     const int* slots, const float* sample_importance, const int* sample_time, const int* sample_type,
                     void* lr_store, void* hr_store, int store_bf16, int capacity, float* means, float* importance,
                     int* time, int* access_count, int* type_id, int flags, void* stream);
/* Rows row0 + j of the fp32 batches = slot idx[j] (j < k, distinct), bf16 widened exactly; access_count[idx[j]] += 1.
 * idx[j] < 0 (a weighted draw that found no eligible slot): that row is zero-filled.  One launch, grid (LR chunks + HR chunks, j). */
int nvq_replay_gather(const void* lr_store, const void* hr_store, int store_bf16, int capacity, long lr_per, long hr_per,
                      const int* idx, int k, float* lr_batch, float* hr_batch, int row0, int* access_count, void* stream);
/* k <= 256 distinct slots with probability proportional to w_i = (1 - recency_weight) * importance_i + recency_weight /
 * (1 + now - time_i), without replacement: the k largest keys log(uniforms[i]) / w_i (Efraimidis-Spirakis; uniforms
 * [capacity] in (0, 1)) over the non-empty slots with w_i > 0 and, for type_filter >= 0, type_id == type_filter.  out_idx in
 * draw order, ties to the lower index, -1 once no eligible slot is left.  One workgroup. */
int nvq_replay_sample_weighted(const float* importance, const int* time, const int* type_id, int capacity, int now,
                               float recency_weight, int type_filter, const float* uniforms, int k, int* out_idx,
                               void* stream);
/* importance[idx[j]] = momentum * importance[idx[j]] + (1 - momentum) * value[j] (two rounded products, one rounded sum);
 * a non-finite value[j] or an idx[j] outside [0, capacity) is skipped.  idx distinct. */
int nvq_replay_update_importance(float* importance, int capacity, const int* idx, const float* value, int k, float momentum,
                                 void* stream);
/* The non-empty slot whose table row [channels] is nearest to query [channels] (Euclidean; lowest index on ties) and that
 * distance; query NULL (channels = 1): the slot with the smallest table value and that value.  No slot: -1, +inf. */
int nvq_replay_nearest(const float* query, const float* table, const int* type_id, int capacity, int channels, int* out_idx,
                       float* out_dist, void* stream);

/* ---- Synchronised BatchNorm (nn.SyncBatchNorm in data-parallel training): every statistics reduction above ends in a
 * finalize step that turns per-block partials into fp64 sums.  These entry points split it at that seam: REDUCE leaves the
 * sums in a caller buffer (fp64), the caller all-reduces that buffer over the ranks, FINISH takes the global sums and reads
 * the pixel count from device memory (no host synchronisation).  With the local sums, reduce + finish is bit-identical to the
 * one-call form.  Buffers (fp64):
 *   forward stats: [G][2][C] = {sum x, sum x^2} per group and channel, then [G] pixel counts (G = 1 for nvq_bn2_*);
 *   backward sums: [G][2][C] = {sum g, sum g*xhat} (g = dy masked by the forward ReLU).
 * dgamma / dbeta are written by the backward reduce phase from the local sums (either may be NULL: a frozen affine); the
 * backward finish phases take the forward's counts (stats + 2*C*G) and compute dx as training-mode BatchNorm does. */
int nvq_bn_stats_reduce(const float* x, int x_ld, int C, int N, int group_images, int H, int W, double* stats,
                        float* workspace, size_t workspace_bytes, int x_bf16, void* stream);
int nvq_bn_stats_finish(const double* stats, int C, int G, float eps, float momentum, const int* order_host,
                        float* mean, float* invstd, float* running_mean, float* running_var, void* stream);
/* nvq_dwpw_forward with its statistics left as sums (the fused bf16, 64-channel forward) */
int nvq_dwpw_forward_sums(const float* in, int in_ld, const nvq_bn_input* bn, const float* dw_weight,
                          const float* pw_weight, float* d, int d_ld, float* p, int p_ld, int N, int group_images,
                          int H, int W, double* stats, float* workspace, size_t workspace_bytes, void* stream);
int nvq_bn_relu_backward_reduce(const float* dy, int dy_ld, const float* x, int x_ld, int C, int N, int group_images,
                                int H, int W, const float* mean, const float* invstd, const float* gamma,
                                const float* beta, double* sums, float* dgamma, float* dbeta, float* workspace,
                                size_t workspace_bytes, int accumulate, int dy_bf16, int x_bf16, void* stream);
int nvq_bn_relu_backward_finish(const float* dy, int dy_ld, const float* x, int x_ld, int C, int N, int group_images,
                                int H, int W, const float* mean, const float* invstd, const float* gamma,
                                const float* beta, const double* sums, const double* count, float* dx, int dx_ld,
                                int dy_bf16, int x_bf16, int dx_bf16, void* stream);
/* the reduce pass of nvq_pw_bn_backward alone, and the pass behind it (dd, dweight; flags: 0 or NVQ_NO_WGRAD) */
int nvq_pw_bn_backward_reduce(const float* dy, int dy_ld, int dy_bf16, const float* p, int p_ld, int N,
                              int group_images, int H, int W, const float* mean, const float* invstd,
                              const float* gamma, const float* beta, double* sums, float* dgamma, float* dbeta,
                              float* workspace, size_t workspace_bytes, void* stream);
int nvq_pw_bn_backward_finish(const float* dy, int dy_ld, int dy_bf16, const float* p, int p_ld, const float* d,
                              int d_ld, int N, int group_images, int H, int W, const float* mean,
                              const float* invstd, const float* gamma, const float* beta, const float* weight,
                              float* dd, int dd_ld, float* dweight, const double* sums, const double* count,
                              float* workspace, size_t workspace_bytes, int flags, void* stream);
int nvq_bn2_stats_reduce(const float* x, int x_ld, int C, long npix, double* stats, float* workspace,
                         size_t workspace_bytes, int bf16, void* stream);
int nvq_bn2_stats_finish(const double* stats, int C, float eps, float momentum, float* mean, float* invstd,
                         float* running_mean, float* running_var, void* stream);
/* dres (with res): the reduce phase writes g there, the finish phase reads it back */
int nvq_bn2_backward_reduce(const float* dy, int dy_ld, const float* x, int x_ld, int C, long npix,
                            const float* mean, const float* invstd, const float* gamma, const float* beta,
                            const float* res, int res_ld, int relu, float* dres, int dres_ld, double* sums,
                            float* dgamma, float* dbeta, float* workspace, size_t workspace_bytes, int bf16,
                            void* stream);
int nvq_bn2_backward_finish(const float* dy, int dy_ld, const float* x, int x_ld, int C, long npix,
                            const float* mean, const float* invstd, const float* gamma, const float* beta,
                            const float* dres, int dres_ld, int relu, const double* sums, const double* count,
                            float* dx, int dx_ld, int bf16, void* stream);

/* ------------------------------------------------------------------ drift detection (csrc/drift.hip)
 * The reference's mlops/drift/detector.py (MMD with an RBF kernel, PSI, the performance monitor) on device-resident samples.
 *
 * nvq_rbf_gram_sum: *out = sum_{i < na, j < nb} exp(-gamma |a_i - b_j|^2) over rows of the row-major fp32 matrices a
 * (a_rows x d) and b (b_rows x d).  a_index / b_index (device, may be NULL): row i of the sum is matrix row a_index[i]
 * (a subsample gathered in the kernel); without one the first na / nb rows.  An index outside [0, rows) reads as a zero row.
 * gamma_dev: one device double, NULL = 1 / d formed in double.  All arithmetic is float64 (inputs widened exactly, a.b and
 * both squared norms on v_mfma_f64_16x16x4_f64, exp in double), one 64 x 64 tile per workgroup with its sum as one double in
 * the workspace (nvq_rbf_gram_workspace_bytes, 8-byte aligned), one finishing block: no atomics, the same bits on every call.
 * symmetric (a == b, same index, na == nb): only tiles on or above the diagonal run and the others are read from their
 * mirror; the result equals the rectangular call on (a, a) bit for bit. */
size_t nvq_rbf_gram_workspace_bytes(int na, int nb, int symmetric);
int nvq_rbf_gram_sum(const float* a, const float* b, const int* a_index, const int* b_index, int na, int nb, int a_rows,
                     int b_rows, int d, const double* gamma_dev, int symmetric, double* out, float* workspace,
                     size_t workspace_bytes, void* stream);
/* sums = {sum K(a, a), sum K(b, b), sum K(a, b)} (device): *score_out = sums[0] / na^2 + sums[1] / nb^2 - 2 sums[2] / (na nb),
 * the biased estimator (diagonals included); *flag_out (one byte) = score > threshold. */
int nvq_mmd_finish(const double* sums, int na, int nb, float threshold, double* score_out, unsigned char* flag_out, void* stream);
/* counts[0 .. nedges - 1) = np.histogram(x, bins = edges)[0] for n fp32 values and 2 .. 11 increasing float64 edges (device):
 * bin i is [e_i, e_{i+1}), the last bin includes its right edge, values outside [e_0, e_last] and NaN are not counted,
 * comparisons in double.  counts is zeroed by the call.  Integer atomics only. */
int nvq_psi_counts(const float* x, long n, const double* edges, int nedges, int* counts, void* stream);
/* *score_out = sum_i (c_i - r_i) log(c_i / r_i), c_i = cur_counts[i] / len_cur + 1e-10, r_i = ref_counts[i] / len_ref + 1e-10
 * (the array lengths, not the counted totals); *flag_out = score > 0.2. */
int nvq_psi_finish(const int* cur_counts, const int* ref_counts, int nbins, long len_cur, long len_ref, double* score_out,
                   unsigned char* flag_out, void* stream);
/* x [B][C][H][W] fp32 -> out [B][2][C][gh][gw]: the mean and the population standard deviation of every cell of a gh x gw
 * grid (gh <= H, gw <= W) with the bounds of adaptive_avg_pool2d: rows floor(i H / gh) .. ceil((i + 1) H / gh).  Sums in
 * double, stored as fp32.  16-byte loads when x is 16-byte aligned and W % 4 == 0; the scalar form gives the same bits. */
int nvq_cell_descriptor(const float* x, int B, int C, int H, int W, int gh, int gw, float* out, void* stream);
/* Push *value (device) into ring [window] at state[0], state = {next position, values held} (device ints, zeroed by the
 * caller before the first push); *mean_out = the mean of the values held, *flag_out = (baseline - mean) / baseline > threshold
 * once `window` values are held, 0 before.  One launch, one block. */
int nvq_metric_window_update(const float* value, float* ring, int* state, int window, float baseline, float threshold,
                             double* mean_out, unsigned char* flag_out, void* stream);

/* ------------------------------------------------------------------ Kolmogorov-Smirnov drift test (csrc/ks.hip, DESIGN.md
 * section 27).  The reference detector's method="ks": scipy.stats.ks_2samp per feature, two-sided, exact p-values.  A set has
 * 1 .. 4096 rows (one column is sorted in LDS); every entry point returns NVQ_EINVAL on a null pointer, a row count outside
 * that range or d < 1 before anything is launched.  NaN inputs are not supported: the answers are then unspecified, but no
 * access leaves its buffer.
 *
 * nvq_sort_columns: out (d x n, feature-major fp32) = every feature's n values in ascending order, from the row-major fp32
 * matrix x (rows x d); index (device, may be NULL): value i of a feature comes from matrix row index[i], an index outside
 * [0, rows) reads as 0; without one the first n rows.  -0.0 is written as +0.0.  Bitonic network over the next power of two,
 * padded with +inf in LDS only. */
int nvq_sort_columns(const float* x, const int* index, int n, int rows, int d, float* out, void* stream);
/* ref_sorted (d x n1), cur_sorted (d x n2): ascending feature-major columns.  With g = gcd(n1, n2), a = n2 / g, b = n1 / g:
 * h_out[f] = max over every value v of either column of |a #{ref <= v} - b #{cur <= v}| (ranks after all copies of v:
 * searchsorted(side='right'), which is what makes ties come out as in scipy), exact integers; d_out[f] = h / lcm(n1, n2),
 * one division in double: the two-sided statistic. */
int nvq_ks_statistic(const float* ref_sorted, const float* cur_sorted, int n1, int n2, int d, int* h_out, double* d_out,
                     void* stream);
/* p_out[f] = P(D >= h[f] / lcm(n1, n2)) under the null hypothesis, exactly (up to rounding): the mass that a walk over the
 * draws of the pooled sample without replacement carries out of the band |a x - b y| < h.  Positive terms only, summed in a
 * fixed order: the bits depend on (n1, n2, h[f]) alone.  h <= 0 gives 1, h > lcm gives 0.  One workgroup per feature. */
int nvq_ks_pvalue(const int* h, int n1, int n2, int d, double* p_out, void* stream);
/* *score_out = d * min_i p[i] (Bonferroni, not clamped), *flag_out (one byte) = score < *threshold_host, compared in double.
 * threshold_host points to one double in HOST memory, read before the call returns (this ABI passes no double by value). */
int nvq_ks_finish(const double* p, int d, const double* threshold_host, double* score_out, unsigned char* flag_out, void* stream);

/* ------------------------------------------------------------------ federated rounds and differential privacy
 * (csrc/federated.hip).  Flat fp32 buffers, sums in double, no atomics; every grid depends on the sizes
 * only and a thread owns whole quads in the 16-byte form (everything 16-byte aligned, stride % 4 == 0) and in the scalar form
 * alike, so a result is the same bits on every call and at every pointer alignment.
 *
 * Noise: z_i for element i of a buffer is Philox4x32-10 (Random123 constants) with key = {seed low, seed high} and counter =
 * {q low, q high, offset low, offset high}, q = i >> 2; the words r0..r3 give u_j = ((r_j >> 8) + 0.5) 2^-24 and elements
 * 4q .. 4q + 3 take sqrt(-2 ln u0) cospi(2 u1), sqrt(-2 ln u0) sinpi(2 u1) and the same from (u2, u3), with the accurate
 * logf / sincospif.  seed and offset are non-negative.  The stream depends on (seed, offset, i) and on nothing else.
 *
 * nvq_fed_delta_norms: clients is a [K][stride] matrix, stride >= n, 1 <= K <= 64; sq[k] = sum_i (x_k[i] - base[i])^2 with the
 * differences and the sums in double (base == NULL: the rows themselves).  One pass reads base once per quad and the K rows,
 * writes per-block partials to the workspace (nvq_fed_workspace_bytes, 8-byte aligned; NVQ_EWORKSPACE when short) and a
 * finishing launch adds them in a fixed order.
 *
 * nvq_fed_aggregate: weights = K device doubles (sample counts, unnormalised), W = their sum in k order; c_k = weights[k] / W *
 * s_k with s_k = min(1, clip_norm / (sqrt(sq[k]) + 1e-6)) when sq != NULL, else 1.  Per element, in double with fma, k ascending:
 * a = sum_k c_k (x_k[i] - base[i]) (base == NULL: 0), v = (float) fma(server_lr, a, base[i]) rounded once, out[i] =
 * fmaf(noise_std, z_i, v); noise_std == 0 skips the noise path: out[i] = v.  FedAvg is base = NULL, sq = NULL, server_lr = 1,
 * noise_std = 0.  out may alias base: every element is read before the same thread writes it.  out must not alias clients.
 * All-zero weights give NaN: the caller checks its sample counts. */
size_t nvq_fed_workspace_bytes(int K, long n);
int nvq_fed_delta_norms(const float* clients, long stride, int K, const float* base, long n, double* sq, float* workspace,
                        size_t workspace_bytes, void* stream);
int nvq_fed_aggregate(const float* clients, long stride, int K, const float* base, const double* weights, const double* sq,
                      float clip_norm, float server_lr, float noise_std, long seed, long offset, long n, float* out,
                      void* stream);
/* Per-slot clipping and noise on a gradient bucket g (16-byte aligned, anything else is NVQ_EINVAL): slot s is numel[s] floats
 * at seg_off[s], a multiple of 4, padded with zeros to the next multiple of 4.  seg_off / seg_numel: S device longs each.
 * chunks: n_chunks device int triples {slot, first quad of the bucket, quads}, sorted by slot, covering every slot's quads once;
 * one block per chunk.  A chunk outside its slot, or of a slot at a misaligned offset, is skipped.
 * nvq_dp_segment_norms: sq[s] = sum of g^2 over slot s, chunk partials in the workspace (n_chunks doubles) added in table order.
 * nvq_dp_clip_noise: coef_s = min(max_norm / (sqrt(sq[s]) + 1e-6), 1) rounded to float; g[i] = fmaf(noise_scale, z_i, g[i] * coef_s)
 * for the numel elements of each slot, q the quad index within the bucket; the padding floats are written as 0 and their draws
 * dropped.  noise_scale == 0 skips the noise path, and a slot with coef_s == 1 is then not written at all. */
int nvq_dp_segment_norms(const float* g, const long* seg_off, const long* seg_numel, int S, const int* chunks, int n_chunks,
                         double* sq, float* workspace, size_t workspace_bytes, void* stream);
int nvq_dp_clip_noise(float* g, const long* seg_off, const long* seg_numel, int S, const int* chunks, int n_chunks,
                      const double* sq, float max_norm, float noise_scale, long seed, long offset, void* stream);

/* ------------------------------------------------------------------ clustered federated learning
 * (csrc/cluster.hip).  The same client matrix and the same rule as above: no atomics, size-only grids,
 * sums in double in a fixed order, the same bits on every call and at every pointer alignment.
 *
 * nvq_fed_update_gram: gram[i * K + j] = sum_t (x_i[t] - base[t]) (x_j[t] - base[t]) as K * K device doubles, 1 <= K <= 64, base
 * == NULL: zeros.  The differences are widened to double before the product; the partial Gram of a block is formed on
 * v_mfma_f64_16x16x4_f64 for the 16 x 16 tiles (i <= j) only, written to the workspace (nvq_fed_gram_workspace_bytes, 8-byte
 * aligned; NVQ_EWORKSPACE when short) and a finishing launch adds the blocks in order and mirrors: gram is symmetric bit for bit.
 *
 * nvq_cluster_gram_kmeans: Lloyd's algorithm on the rows behind a Gram matrix, from the Gram alone, one workgroup, 1 <= C <= 8,
 * C <= K.  d(k, c) = G_kk - (2 / |S_c|) sum_{j in S_c} G_kj + (1 / |S_c|^2) sum_{i, j in S_c} G_ij, +inf for an empty cluster (it
 * stays empty).  init: C device ints, distinct row indices (one outside [0, K) gives an empty cluster), or NULL: farthest-first,
 * the first seed the row with the largest G_kk, each next one the row that maximises its minimum distance to the seeds so far,
 * ties to the lowest index.  Rows go to the nearest seed, then up to max_iter sweeps reassign every row to its nearest centroid
 * (ties to the lowest cluster) until no label changes; n_iter = the sweeps made.  labels: K ints, counts: C ints, inertia: one
 * double, the sum of d(k, labels[k]) for the final labels, n_iter: one int, all on the device.
 *
 * nvq_fed_aggregate_clusters: labels = K device ints; for c < C, with S_c = {k : labels[k] == c}, W_c = sum of weights over S_c in
 * ascending k and c_k = weights[k] / W_c * s_k (s_k from sq and clip_norm as in nvq_fed_aggregate): out[c * out_stride + i] =
 * the value nvq_fed_aggregate gives for the rows of S_c in ascending k with base = bases + c * base_stride and the noise stream
 * (seed, offset + c).  base_stride == 0: one shared base; bases == NULL: zeros.  sq != NULL needs base_stride == 0.  An empty
 * cluster's row is its base (plus noise); a label outside [0, C) leaves the client out.  out may be bases when out_stride ==
 * base_stride (or C == 1); out must not alias clients.  Members whose weights are all zero give NaN in that row. */
size_t nvq_fed_gram_workspace_bytes(int K, long n);
int nvq_fed_update_gram(const float* clients, long stride, int K, const float* base, long n, double* gram, float* workspace,
                        size_t workspace_bytes, void* stream);
int nvq_cluster_gram_kmeans(const double* gram, int K, int C, const int* init, int max_iter, int* labels, int* counts,
                            double* inertia, int* n_iter, void* stream);
int nvq_fed_aggregate_clusters(const float* clients, long stride, int K, const int* labels, int C, const float* bases,
                               long base_stride, const double* weights, const double* sq, float clip_norm, float server_lr,
                               float noise_std, long seed, long offset, long n, float* out, long out_stride, void* stream);

/* ------------------------------------------------------------------ Byzantine-robust aggregation
 * (csrc/robust.hip).  The same client matrix and the same rule as above: no atomics, size-only grids, sums
 * in double in a fixed order, the same bits on every call and at every pointer alignment.
 *
 * A row k is live when weights == NULL or weights[k] > 0 (K device doubles); m = the number of live rows.  A row that is not live
 * is never read, so a zero-weight row of NaN does not reach the result (it would through 0 * NaN in nvq_fed_aggregate).
 *
 * nvq_fed_trimmed_aggregate: per element i the live rows are sorted ascending by x_k[i] (NaN after +inf whatever its sign bit, as
 * np.sort; -0.0 and +0.0 in either order), t = min(trim, (m - 1) / 2), a = the sum of d_k = (double) x_k[i] - (double) base[i] over
 * the sorted positions t .. m - 1 - t, added in that order in double, divided by m - 2 t (m == 0: a = 0); v = (float) fma(server_lr,
 * a, base[i]) rounded once, out[i] = fmaf(noise_std, z_i, v) with the noise stream of nvq_fed_aggregate ("Noise" above; noise_std
 * == 0 skips the noise path).  base == NULL: zeros.  trim = 0 is the unweighted mean of the live rows; trim >= (K - 1) / 2, for
 * which NVQ_FED_TRIM_MEDIAN stands, the coordinate-wise median (the middle value, or the mean of the two middle values).
 * 1 <= K <= 64.  out may alias base; out must not alias clients.
 *
 * nvq_fed_krum_select: gram = the K * K doubles nvq_fed_update_gram leaves.  D_ij = max(0, G_ii + G_jj - 2 G_ij) over live i != j,
 * a NaN distance replaced by +inf; c = min(max(m - num_byzantine - 2, 1), m - 1); scores[i] = the sum of the c smallest D_ij,
 * added ascending in double (one live row: 0), +inf for a row that is not live.  order = the live rows by (score, index)
 * ascending, NaN scores last, then the other rows by index; out_weights[k] = 1 for the first min(num_selected, m) rows of order,
 * else 0.  One workgroup.  nvq_fed_trimmed_aggregate with trim = 0 and weights = out_weights then averages the selected rows. */
#define NVQ_FED_TRIM_MEDIAN 64
int nvq_fed_trimmed_aggregate(const float* clients, long stride, int K, const float* base, const double* weights, int trim,
                              float server_lr, float noise_std, long seed, long offset, long n, float* out, void* stream);
int nvq_fed_krum_select(const double* gram, int K, const double* weights, int num_byzantine, int num_selected,
                        double* out_weights, double* scores, int* order, void* stream);

/* ------------------------------------------------------------------ Federated optimisation: FedOpt server rules and the FedProx
 * gradient (csrc/fedopt.hip).  The same client matrix and the same rule as above: one launch each, no
 * atomics, no workspace, size-only grids, the same bits on every call and at every pointer alignment.
 *
 * nvq_fed_server_opt: the sweep of nvq_fed_aggregate with a stateful server step.  Per element, everything in double: D = sum_k
 * c_k (x_k[i] - base[i]) with c_k, the fma chain and its order exactly as in nvq_fed_aggregate; mp = m[i] and vp = v[i] widened;
 * the hyper-parameters are the given floats widened.
 *   NVQ_FED_OPT_AVGM     m' = fma(beta1, mp, D), step = m'; v is neither read nor written and may be NULL
 *   the adaptive rules   m' = fma(beta1, mp, (1 - beta1) D), d2 = D * D rounded on its own, and
 *   NVQ_FED_OPT_ADAGRAD  v' = vp + d2
 *   NVQ_FED_OPT_ADAM     v' = fma(beta2, vp, (1 - beta2) d2)
 *   NVQ_FED_OPT_YOGI     v' = vp - (1 - beta2) d2 sign(vp - d2), sign(0) = 0
 *                        step = m' / (sqrt(v') + tau)
 * out[i] = fmaf(noise_std, z_i, (float) fma(server_lr, step, base[i])) with the noise stream of nvq_fed_aggregate (noise_std == 0
 * skips the noise path), m[i] = (float) m', v[i] = (float) v': the step uses the unrounded m' and v', so each stored value is the
 * double chain rounded once.  AVGM with beta1 = 0 and m finite gives the bits of nvq_fed_aggregate.  base, weights, m and out
 * are required, v for the adaptive rules; 0 <= beta1, beta2 < 1; tau > 0 for the adaptive rules; v >= 0 is the caller's (the
 * usual start is tau^2).  out may alias base; out, m and v must not alias clients or each other.  K = 1 with weights = {1}
 * steps from base towards a vector that another rule has aggregated.
 *
 * nvq_fed_prox_grad: grad[i] = (float) fma((double) mu, (double) theta[i] - (double) anchor[i], (double) grad[i]) in place, the
 * gradient of mu / 2 |theta - anchor|^2 added to a flat gradient bucket; theta and anchor are only read.  mu >= 0; mu == 0
 * launches nothing. */
#define NVQ_FED_OPT_AVGM 0
#define NVQ_FED_OPT_ADAGRAD 1
#define NVQ_FED_OPT_ADAM 2
#define NVQ_FED_OPT_YOGI 3
int nvq_fed_server_opt(const float* clients, long stride, int K, const float* base, const double* weights, const double* sq,
                       float clip_norm, int rule, float server_lr, float beta1, float beta2, float tau, float* m, float* v,
                       float noise_std, long seed, long offset, long n, float* out, void* stream);
int nvq_fed_prox_grad(float* grad, const float* theta, const float* anchor, long n, float mu, void* stream);

/* ------------------------------------------------------------------ Compressed client updates: top-k sparsification with error
 * feedback and QSGD stochastic quantisation (csrc/compress.hip).  The same client matrix, changed in place
 * row by row, so every rule above works on the compressed rows unchanged.  Integer counters only (LDS histograms merged by integer
 * atomics), no float atomics: the same bits on every call and at every pointer alignment.
 *
 * nvq_fed_compress: x = row r of clients, b = base (NULL: zeros), e = row slots[r] of residual (an [M][residual_stride] matrix;
 * slots = K device ints, distinct and in range, which is the caller's to guarantee; NULL: row r; residual == NULL: no e).  Per
 * coordinate i, every step one correctly rounded IEEE operation or exact:
 *   1. a_i = (float) (((double) x_i - (double) b_i) + (double) e_i); without a residual there is no + e_i.
 *   2. key_i = the 31 magnitude bits of a_i as an unsigned integer; every NaN has the largest key, after inf.
 *   3. 1 <= k < n: T = the k-th largest key of the row, i is kept iff key_i >= T; ties at T are all kept, so kept[r] >= k, and
 *      kept[r] == k when the k-th and (k + 1)-th magnitudes differ.  k == 0 or k >= n: everything is kept, kept[r] = n.  The
 *      selection is exact (a radix select on the keys).
 *   4. levels = s in 1 .. 32767 (0: off): scale = the float whose key is the row's largest key.  scale 0, inf or NaN: the row is
 *      not quantised, c_i = a_i.  Else for a kept i: u_i = ((w_i >> 8) + 0.5) 2^-24 with w_i word i & 3 of Philox quad i >> 2 of
 *      the stream (seed, offset + r) ("Noise" above), t = (double) |a_i| * s / (double) scale (the product, then the quotient),
 *      xi_i = floor(t + u_i), c_i = (float) (sgn(a_i) xi_i (double) scale / s) (the product, then the quotient).  E[xi] = t.
 *      levels == 0: c_i = a_i.
 *   5. kept: x'_i = (float) ((double) b_i + (double) c_i); dropped: x'_i = b_i.
 *   6. e'_i = (float) ((double) a_i - ((double) x'_i - (double) b_i)), stored as 0 when it is not finite.
 * clients receives x', the residual row e' (rows that slots does not name are not touched), kept (K device ints, may be NULL)
 * the number of kept coordinates per row.  1 <= K <= 64, stride >= n, residual_stride >= n, k >= 0, n < 2^31.  Launches: with
 * top-k three counting passes (digits of 11, 10 and 10 bits; the first stores a into the residual row, so the later ones read
 * one stream) and the sweep; without it one pass for the row maxima (only with levels > 0) and the sweep.  The workspace
 * (nvq_fed_compress_workspace_bytes, 4-byte aligned; NVQ_EWORKSPACE when short) is cleared on the stream.  k == 0 && levels == 0
 * && residual == NULL changes nothing and fills kept with n.  base, residual and workspace must not alias clients. */
size_t nvq_fed_compress_workspace_bytes(int K, long n);
int nvq_fed_compress(float* clients, long stride, int K, const float* base, long n, long k, int levels, float* residual,
                     long residual_stride, const int* slots, long seed, long offset, int* kept, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ ABR agent: vectorised streaming environment, fused act,
 * GAE and the PPO loss (csrc/abr.hip).  No atomics; sums in double in a fixed order; plain vector stores.
 *
 * Draws: Philox4x32-10 as in "Noise" above with key = {seed low, seed high} and counter = {e low, e high, t low,
 * (t high & 0xFFFFFF) | stream << 24} for environment e and its draw counter t = counters[e] (t < 2^56); the words r0..r3 give
 * u_j = ((r_j >> 8) + 0.5) 2^-24 in double.  Stream 0 is the environment: bandwidth factor 0.8 + 0.4 u0, content complexity of
 * the returned observation 0.3 + 0.5 u1 and, when the step ends the episode (and in nvq_abr_env_reset), the new bandwidth
 * 2 + 13 u2 and the reset observation's complexity 0.3 + 0.5 u3.  Stream 1 is the policy: head j samples with u_j.  Both
 * environment calls add one to every counters[e].
 *
 * state: N rows of 8 doubles {buffer level, bandwidth, battery, last quality, last VMAF, step count, total rebuffer, episode
 * return}; counters: N longs; params: 2 device doubles {segment duration, buffer size}; obs: N rows of 7 floats.  One thread per
 * environment, float64 in the order of operations of the single-environment step, without contraction.  An action outside its
 * range is clamped into it.  An environment whose step ends its episode (step count >= max_steps: terminated; battery <= 0:
 * truncated) is reset in the same call: reward, flags and info are those of the finished step, obs is the reset observation.
 * info (optional): 5 rows of N doubles {vmaf, rebuffer, bandwidth, buffer, episode return}.  reward_f32 / done_f32 (optional): the
 * reward and (terminated | truncated) as floats, e.g. a row of a rollout.  finished (optional): N pairs {sum of finished episode
 * returns, finished episodes}, added to by the environment's own thread.  1 <= nq <= 16 ladder entries (kbps), enh_levels >= 2.
 *
 * nvq_abr_act: the actor-critic forward and sampling in one launch.  params_host: 16 device pointers {W1, b1, W2, b2, W3, b3,
 * Wh0, bh0, .., Wh3, bh3, Wv, bv}, nn.Linear layouts ([out][in] weights, 16-byte aligned), unused entries NULL; dims_host: 9 ints
 * {hidden layers, w1, w2, w3, heads, n0, n1, n2, n3}.  Supported (nvq_abr_act_supported; anything else is NVQ_EINVAL): obs_dim <=
 * 32, 1 to 3 hidden layers of a width that is a multiple of 32 in [32, 512], 1 to 4 heads, at most 32 head outputs with the
 * value; any B >= 1.  The linears run on v_mfma_f32_16x16x4_f32; each head's log-softmax is x - (m + logf(sum expf(x - m))).
 * Sampling: the CDF of expf(log-softmax) is added in index order in fp32, the action is the first k with u < cdf_k, else the last;
 * the draw of row i is (e = i, t = counters[i]) on stream 1.  deterministic != 0 or counters == NULL: the first index of the
 * maximum.  actions: B rows of `heads` ints; log_prob: the sum over the heads of the log-probability of the action taken;
 * head_out (optional): B rows of the P = n0 + .. + 1 raw head outputs, the value last.
 *
 * nvq_abr_gae: rewards / values / dones / returns / advantages are [T][N] floats, one thread per environment from t = T - 1 down:
 * delta = r + gamma v_next (1 - done) - v, gae = delta + gamma lam (1 - done) gae, returns = gae + v, v_next of the last step =
 * last_values.  nvq_abr_adv_stats: stats = {mean, unbiased standard deviation} of M floats as 2 device doubles, one workgroup.
 *
 * nvq_ppo_loss: head_outputs / grad are M rows of P floats (the heads' logits, then the value), actions M rows of n_heads ints.
 * Per sample, in double: A = (adv - stats[0]) / (stats[1] + 1e-8), ratio = exp(new log-prob - old), policy term
 * -min(ratio A, clamp(ratio, 1 - clip, 1 + clip) A), value term (v - return)^2, the heads' entropies.  out = 6 device doubles
 * {loss, policy loss, value loss, entropy, approximate KL = mean((ratio - 1) - log ratio), clip fraction = mean(|ratio - 1| >
 * clip)} with loss = policy + value_coef * value - entropy_coef * entropy, means over M; grad = d loss / d head_outputs rounded
 * once to fp32.  Block partials go to the workspace (nvq_ppo_loss_workspace_bytes, 8-byte aligned; NVQ_EWORKSPACE when short)
 * and a finishing launch adds them in block order.  P <= 64. */
int nvq_abr_env_reset(double* state, long* counters, float* obs, const double* params, int nq, int max_steps, long seed, int N,
                      void* stream);
int nvq_abr_env_step(double* state, long* counters, const int* actions, const int* bitrates_host, int nq, int enh_levels,
                     int max_steps, const double* params, long seed, int N, float* obs, double* reward,
                     unsigned char* terminated, unsigned char* truncated, double* info, float* reward_f32, float* done_f32,
                     double* finished, void* stream);
int nvq_abr_act_supported(int obs_dim, const int* dims_host);
int nvq_abr_act(const float* obs, int B, int obs_dim, const void* params_host, const int* dims_host, const long* counters,
                long seed, int deterministic, int* actions, float* log_prob, float* value, float* head_out, void* stream);
int nvq_abr_gae(const float* rewards, const float* values, const float* dones, const float* last_values, float gamma, float lam,
                int T, int N, float* returns, float* advantages, void* stream);
int nvq_abr_adv_stats(const float* adv, long M, double* stats, void* stream);
size_t nvq_ppo_loss_workspace_bytes(long M);
int nvq_ppo_loss(const float* head_outputs, const int* actions, const float* old_log_probs, const float* advantages,
                 const double* adv_stats, const float* returns, long M, const int* heads_host, int n_heads, float clip_ratio,
                 float value_coef, float entropy_coef, float* grad, double* out, double* workspace, size_t workspace_bytes,
                 void* stream);

/* ------------------------------------------------------------------ Gradient Episodic Memory (csrc/gem.hip, DESIGN.md
 * section 32).  GEM (Lopez-Paz & Ranzato 2017) keeps one reference gradient per earlier task: refs is a [T][stride] fp32 matrix,
 * 1 <= T <= 15, stride >= n, and g the step's gradient, n floats.  The flat-buffer rule holds: no atomics, size-only grids, sums
 * in double in a fixed order, the same bits on every call and at every pointer alignment (4-byte aligned pointers suffice).
 *
 * nvq_gem_gram: gram = 16 x 16 device doubles; gram[i * 16 + j], i, j <= T, = the inner product of rows i and j, index T standing
 * for g.  Every factor is widened to double before the product (v_mfma_f64_16x16x4_f64); block partials go to the workspace
 * (flat blocks x 256 doubles, <= 2 MiB, 8-byte aligned; NVQ_EWORKSPACE when short) and a finishing launch adds them in block
 * order and mirrors: gram is symmetric bit for bit, and zero outside (T + 1) x (T + 1).  `accumulate` adds to the entries that are
 * there (the next segment of the same model).
 *
 * nvq_gem_solve: q = gram[.][T], P = gram[0..T)[0..T) + ridge I with ridge = eps, or eps * max_t gram[t][t] with eps_relative.
 * When some q_t < 0: v = argmin 1/2 v'Pv + q'v subject to v >= margin, by a primal active-set method in double on one
 * workgroup, at most 64 Cholesky solves.  v = 16 device doubles, all zero when no q_t < 0 (a NaN compares false), when T == 0 or
 * when a used gram entry is not finite.  stats = 8 device doubles: [0] number of q_t < 0, [1] number of v_t > margin, [2] solves,
 * [3] status (0 solved, 1 cap reached: the last feasible iterate is used, 2 non-finite input: no projection), [4] += 1 when this
 * call projects (the caller zeroes it once), [5] g.g, [6] g'.g' of the projected gradient from the Gram alone, [7] min_t cos(g,
 * r_t) (a zero row counts as 0).
 *
 * nvq_gem_project: g[i] = (float)((double)g[i] + sum_t v[t] (double)refs[t][i]), t ascending, every term one fma in double.  v all
 * zero leaves g untouched (bit-identical); a row with v[t] == 0 is not read. */
int nvq_gem_gram(const float* refs, long stride, int T, const float* g, long n, double* gram, int accumulate, float* workspace,
                 size_t workspace_bytes, void* stream);
int nvq_gem_solve(const double* gram, int T, float margin, float eps, int eps_relative, double* v, double* stats, void* stream);
int nvq_gem_project(float* g, const float* refs, long stride, int T, long n, const double* v, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NVQ_H */
