/*
 * neube_hip.h -- C ABI of the MI355X (gfx950) NeuBE generator kernels.
 *
 * This is the drop-in boundary for the reference's native plugin layer.  In the reference the
 * generator's arithmetic bottoms out in two pybind11/CUDA plugins plus cuDNN:
 *
 *   bias_act_plugin.bias_act(x,b,xref,yref,dy,grad,dim,act,alpha,gain,clamp)
 *       thirdparty/stylegan2_ada_pytorch/torch_utils/ops/bias_act.cpp:32-91  (kernel bias_act.cu:23-147)
 *   upfirdn2d_plugin.upfirdn2d(x,f,upx,upy,downx,downy,padx0,padx1,pady0,pady1,flip,gain)
 *       thirdparty/stylegan2_ada_pytorch/torch_utils/ops/upfirdn2d.cpp:16-94 (kernels upfirdn2d.cu:29-200)
 *   torch.nn.functional.conv2d / conv_transpose2d (cuDNN) via
 *       thirdparty/stylegan2_ada_pytorch/torch_utils/ops/conv2d_gradfix.py:35-43
 *   loaded lazily by torch_utils/custom_ops.py:46-124 (JIT nvcc build).
 *
 * Here they are replaced by one ahead-of-time hipcc-built shared library with plain-C entry
 * points: raw device pointers, integer sizes, scalar parameters and the HIP stream to launch on.
 * No torch types cross this boundary.  All tensors are dense, contiguous, float32, NCHW.
 * Outputs are caller-allocated.  Every function returns 0 on success and a negative NB_E* code on
 * failure; nb_last_error() then returns a thread-local message.  Functions only enqueue work on
 * `stream` (no allocation, no synchronisation) and are therefore capturable into a hipGraph.
 *
 * `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).
 */
#ifndef NEUBE_HIP_H
#define NEUBE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NB_OK            0
#define NB_EINVAL       -1   /* bad argument (shape, null pointer, unsupported mode) */
#define NB_ELAUNCH      -2   /* the HIP runtime rejected a launch */
#define NB_EUNSUPPORTED -3

/* activation codes = the reference's cuda_idx (bias_act.py:22-32) */
#define NB_ACT_LINEAR  1
#define NB_ACT_RELU    2
#define NB_ACT_LRELU   3
#define NB_ACT_TANH    4
#define NB_ACT_SIGMOID 5
#define NB_ACT_ELU      6
#define NB_ACT_SELU     7
#define NB_ACT_SOFTPLUS 8
#define NB_ACT_SWISH    9

const char* nb_last_error(void);
int nb_abi_version(void);

/* ---- standalone operator parity with the reference plugins ------------------------------- */

/* y = clamp(act(x + b[(i / step_b) % size_b]) * gain, +-clamp); forward (grad=0) of
 * bias_act.cpp:32-91.  size_b = 0 -> no bias.  clamp < 0 -> no clamping.  x and y may alias. */
int nb_bias_act_f32(const float* x, const float* b, float* y, int64_t size_x, int size_b, int step_b,
                    int act, float alpha, float gain, float clamp, void* stream);

/* The plugin's full entry (bias_act.cpp:32 `bias_act(x, b, xref, yref, dy, grad, dim, act, alpha, gain, clamp)`,
 * kernel bias_act.cu:23-147) with the gradient modes the reference's autograd functions call
 * (bias_act.py:155-204):
 *   grad 0: forward as above (xref, yref, dy ignored).
 *   grad 1: x = incoming gradient, returns x * act'(.) * gain, zero where the forward output was clamped.
 *   grad 2: x = gradient w.r.t. the grad-1 result, dy = the original incoming gradient; returns
 *           x * dy * act''(.) * gain (identically zero for linear / relu / lrelu).
 * yref = the forward output (needed by every activation but linear-without-clamp and swish),
 * xref = the forward input, bias not yet added (needed by swish only); unused ones may be NULL. */
int nb_bias_act_grad_f32(const float* x, const float* b, const float* xref, const float* yref, const float* dy,
                         float* y, int64_t size_x, int size_b, int step_b, int grad, int act, float alpha,
                         float gain, float clamp, void* stream);

/* upfirdn2d.cpp:16-94 forward on a contiguous [major, in_h, in_w] stack of planes (major = N*C):
 * zero-insert by (upx,upy), pad/crop, correlate with f[f_h,f_w] (flipped unless `flip`), scale by
 * gain, keep every (downx,downy)-th sample.  y is [major, out_h, out_w] with
 * out_w = (in_w*upx + padx0 + padx1 - f_w + downx) / downx (same for h). */
int nb_upfirdn2d_f32(const float* x, const float* f, float* y, int major, int in_h, int in_w,
                     int f_h, int f_w, int upx, int upy, int downx, int downy,
                     int padx0, int padx1, int pady0, int pady1, int flip, float gain, void* stream);

/* ---- gradient building blocks (row f4; csrc/nb_grad.hip) ------------------------------------------ */

/* Generic fp32 convolution (cross-correlation, zero padding), what conv2d_gradfix.py:107-168 takes from cuDNN for the
 * gradient w.r.t. the input of a strided conv:
 *   y[n,co,oy,ox] = out_scale[n,co] * sum_{ci,a,b} (x[n,ci,oy*stride+a-pad,ox*stride+b-pad] * in_scale[n,ci]) * w[co,ci,a,b]
 * x [n,c_in,h,wd], w [c_out,c_in,kh,kw] (kh, kw <= 7), y [n,c_out,ho,wo], ho = (h + 2 pad - kh)/stride + 1; the per-sample
 * scales may be NULL. */
int nb_conv2d_f32(const float* x, const float* w, const float* in_scale, const float* out_scale, float* y, int n,
                  int c_in, int h, int wd, int c_out, int kh, int kw, int stride, int pad, void* stream);

/* Weight-gradient correlation of a 3x3 conv: a[n,cu,cv,ka,kb] = sum_{i,j} u[n,cu,i*stride+ka-pad,j*stride+kb-pad] * v[n,cv,i,j]
 * (zero outside u); a [n,cu,cv,3,3] is overwritten (partial sums are added atomically: the last bits depend on the
 * order). */
int nb_conv2d_wgrad_f32(const float* u, const float* v, float* a, int n, int cu, int hu, int wu, int cv, int hv, int wv,
                        int stride, int pad, void* stream);

/* The same on the f16 matrix cores with split (hi/lo) operands: scales = 2 floats in device memory, powers of two that bring
 * max|u| and max|v| near 2^10 (gradients may sit far below the f16 range); the result is divided by their product. */
int nb_conv2d_wgrad_h3(const float* u, const float* v, const float* scales, float* a, int n, int cu, int hu, int wu, int cv,
                       int hv, int wv, int stride, int pad, void* stream);

/* The same without atomics (the form the training path uses): every workgroup stores its partial block, one more launch
 * adds the blocks in a fixed order -- the result is reproducible and a is not zero-filled first.  sum_n != 0 also sums over
 * the samples: a is [cu,cv,3,3] (what a plain convolution's weight gradient needs; conv2d_gradfix.py:129-137).
 * ws: device scratch of at least nb_conv2d_wgrad_h3_ws_bytes(...) bytes, 16-byte aligned (may be NULL when that is 0). */
long long nb_conv2d_wgrad_h3_ws_bytes(int n, int cu, int cv, int hv, int sum_n);
int nb_conv2d_wgrad_h3_ws(const float* u, const float* v, const float* scales, int scales_are_absmax, float* a, float* ws,
                          long long ws_bytes, int sum_n, int n, int cu, int hu, int wu, int cv, int hv, int wv, int stride, int pad,
                          void* stream);
/* scales_are_absmax != 0: `scales` holds max|u|, max|v| (the two slots nb_absmax_f32 fills) and the kernel derives the powers
 * of two itself. */

/* The tail of modulated_conv2d's backward pass (what autograd spells out as einsums and element-wise passes in the reference,
 * training/networks.py:30-88 differentiated): dd[n,o] = sum_pix dy (y - noise) (noise: NULL, one shared plane with stride 0, or one
 * plane per sample); and, with A[n,o,c,3,3] the per-sample weight-gradient correlation (element strides given: the wgrad kernels
 * leave it as [n][c][o][9] for up = 1 and [n][o][c][9] for up = 2), s the styles, dq = d(loss)/d(sum under the demodulation rsqrt)
 * or NULL:  dW[o,c,t] = sum_n s A + 2 W sum_n dq s^2,   ds[n,c] = sum_{o,t} W A + 2 s sum_o dq sum_t W^2.  dW or ds may be NULL. */
int nb_modconv_bwd_dot_f32(const float* dy, const float* y, const float* noise, long long noise_stride_n, float* out, int n, int o,
                           int hw, void* stream);
int nb_modconv_bwd_finish_f32(const float* A, long long a_stride_n, long long a_stride_o, long long a_stride_c, const float* s,
                              const float* W, const float* dq, float* dW, float* ds, int n, int o, int c, void* stream);

/* Range scaling of the split-f16 training operators (no counterpart in the reference, whose cuDNN path computes in fp32 /
 * fp16 directly): slots = two 4-byte device words, zero-filled by the caller; afterwards slots[0] = max(|a|, |b|) and
 * slots[1] = max|c| as float bit patterns (a, b, c may be NULL with a zero count). */
int nb_absmax_f32(const float* a, long long na, const float* b, long long nb, const float* c, long long nc, void* slots, void* stream);
/* nb_pack_h2_f32 with the scale derived on the device: out = H2((x1 ++ x2) * scale[n,c] * k), k = the power of two that
 * brings slots[0] * slots[1] near `target`; also dco_out[i] = dco_in[i] / k for i < dco_count (may be 0). */
int nb_pack_h2_ranged_f32(const float* x1, int c1, const float* x2, int c2, const float* scale, void* out_h2, int n, int hw,
                          const void* slots, float target, const float* dco_in, float* dco_out, int dco_count, void* stream);

/* ---- generator path ---------------------------------------------------------------------- */

/* MappingNetwork.forward (training/networks.py:255-290) for c_dim = 0, without the broadcast:
 * w[n,:] = FC_{L-1}(...FC_0(z * rsqrt(mean(z^2)+1e-8))), each FC = lrelu(x W^T * lr_mul/sqrt(in) + b*lr_mul)*sqrt2.
 * fc_w: layer 0 [w_dim, z_dim] followed by layers 1.. [w_dim, w_dim]; fc_b: [L, w_dim].
 * z_dim, w_dim <= 512. */
int nb_mapping_f32(const float* z, const float* fc_w, const float* fc_b, float* w_out, int n, int z_dim,
                   int w_dim, int num_layers, float lr_mul, void* stream);

/* The same with the broadcast of networks.py:278-280 written by the kernel: ws_out [n, num_ws, w_dim]. */
int nb_mapping_ws_f32(const float* z, const float* fc_w, const float* fc_b, float* ws_out, int n, int z_dim,
                      int w_dim, int num_layers, float lr_mul, int num_ws, void* stream);

/* One entry of the per-layer table consumed by nb_styles_f32 / nb_noise_f32 (device memory, built
 * once when weights are packed).  Pointers are device addresses. */
typedef struct NbLayerDesc {
    const float* affine_w;   /* [c_aff, w_dim]  FullyConnectedLayer.weight of the layer's affine */
    const float* affine_b;   /* [c_aff] */
    const float* wsq;        /* [c_in, c_out]   sum_k W[o,i,k]^2 (transposed), NULL -> no demodulation */
    float*       styles;     /* out [n_max, c_aff]  affine(w) * style_scale (entries < n_plain are NOT scaled) */
    float*       dcoefs;     /* out [n_max, c_out]  rsqrt(sum_i (styles^2 * wsq) + 1e-8), unused when wsq NULL */
    const float* noise_const;/* [res, res] or NULL */
    const float* noise_lin;  /* [res] = noise_grid[0, :, 0, 0] (torch.linspace(0,1,res)) */
    float*       noise_out;  /* out [n_max or 1, res, res] = (shifted) noise_const * noise_strength */
    const float* noise_strength; /* [1] */
    int32_t c_aff;           /* affine outputs (= c_in, or c_in + 9 for the triad ToRGB) */
    int32_t n_plain;         /* leading affine outputs that are not styles (9 color scalars for ToRGB, else 0) */
    int32_t c_out;
    int32_t w_index;         /* which ws[:, w_index, :] feeds this layer */
    int32_t res;             /* output resolution of the layer (noise size) */
    float   style_scale;     /* 1 for conv layers, 1/sqrt(c_in) for ToRGB (networks.py:460) */
    int32_t pad_[2];
} NbLayerDesc;

/* For every layer l < n_layers and sample n: styles = affine_l(ws[n, w_index_l]) (weight_gain
 * 1/sqrt(w_dim), bias_gain 1: networks.py:106-118) and the demodulation coefficients
 * (networks.py:59-62 in the algebraically equal form d = rsqrt(sum_i s_i^2 * sum_k W_oik^2 + 1e-8)). */
int nb_styles_f32(const NbLayerDesc* layers_dev, int n_layers, const float* ws, int num_ws, int w_dim, int n,
                  void* stream);

/* Same results up to fp32 summation order, latency-oriented launch shape (the batch-1 step starts with it): needs
 * w_dim % 16 == 0, every layer's c_out % 4 == 0 and c_aff <= 1024 (the squared styles live in LDS; nb_styles_f32 takes
 * any c_aff), and 16-byte aligned affine_w / wsq. */
int nb_styles_fast_f32(const NbLayerDesc* layers_dev, int n_layers, const float* ws, int num_ws, int w_dim, int n,
                       void* stream);

/* nb_styles_fast_f32 and nb_noise_f32 (per-sample shifted noise: exactly one of norm_pos / positions) in ONE launch -
 * the two are independent, and at batch 1 a launch costs more than either computes. */
int nb_styles_noise_f32(const NbLayerDesc* layers_dev, int n_layers, const float* ws, int num_ws, int w_dim,
                        const float* norm_pos, const int64_t* positions, int img_resolution, int n, void* stream);

/* Stand-alone demodulation coefficients for one layer (networks.py:59-62 in the form above):
 * dcoefs[n,o] = rsqrt(sum_i styles[n,i]^2 * wsq[i,o] + 1e-8); styles [n,c_in], wsq [c_in,c_out]. */
int nb_demod_coefs_f32(const float* styles, const float* wsq, float* dcoefs, int n, int c_in, int c_out,
                       void* stream);

/* Constant-noise inputs of all layers in one launch (networks.py:371-382).
 *   norm_pos == NULL && positions == NULL: noise_out[0] = noise_const * strength (shared by the batch).
 *   positions != NULL: [n,2] int64 (y,x) patch positions; the kernel forms the reference's
 *       (positions % img_resolution) / (img_resolution - 1) (networks_modified.py:351-353) itself, with
 *       python-style modulo and correctly rounded float32 division, so that it is bit-identical to the
 *       reference's CPU arithmetic (the wrapped coordinate is discontinuous: 1 ulp moves a noise row).
 *   norm_pos != NULL: [n,2] float32 already-normalised positions (the `norm_noise_positions` kwarg).
 * noise_out[n] is the bilinear, wrapped resampling of SURVEY note C.  Layers whose noise_const is
 * NULL are skipped.  max_res = largest `res` in the table.  The reference's noise_buffers override
 * (networks_modified.py:163-165) is expressed by passing a table with replaced noise_const pointers. */
int nb_noise_f32(const NbLayerDesc* layers_dev, int n_layers, int max_res, const float* norm_pos,
                 const int64_t* positions, int img_resolution, int n, void* stream);

/* Seeded random noise of all layers in one launch: SynthesisLayer's noise_mode 'random' (training/networks.py:369-370:
 * torch.randn([n, 1, res, res]) * noise_strength) with a counter-based generator in place of torch's global one, so that the
 * draw is a pure function of (seed, sample, layer, pixel): the same sample gets the same noise at any batch size, on any rank,
 * from Python or C, and in every replay of a captured graph.  Positions play no part, as in the reference's random mode.
 * For table row i (layer l = first_layer + i: the index in the generator's layer list, absolute even when a table + lo is
 * passed), sample k < n and pixel quad q (pixels 4q .. 4q+3 of the row-major res * res image):
 *     s = offset + k                                                  (uint64, wraps)
 *     (x0, x1, x2, x3) = Philox4x32-10(counter = (q, l, lo32(s), hi32(s)), key = (lo32(seed), hi32(seed)))
 *         (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds)
 *     pair(a, b): u1 = ((a >> 8) + 1) * 2^-24 in (0, 1], u2 = (b >> 8) * 2^-24 in [0, 1)   (both exact in fp32)
 *                 r = sqrtf(-2 logf(u1)); (z_even, z_odd) = (r cospif(2 u2), r sinpif(2 u2))   (accurate library functions)
 *     pixels 4q, 4q+1 = pair(x0, x1); pixels 4q+2, 4q+3 = pair(x2, x3)
 *     noise_out[k, pixel] = z * noise_strength[0]       (one fp32 multiply; noise_strength == NULL: z itself)
 * So sample k at offset o is sample 0 at offset o + k.  Rows whose noise_out is NULL are skipped (the ToRGB row); only res,
 * noise_out and noise_strength of a row are read.  res * res need not be a multiple of 4.  state_dev: NULL, or a device pointer
 * to {seed, offset}; then the kernel reads the two from there and ignores the by-value arguments (a captured graph draws fresh
 * noise by writing 16 bytes before a replay).  Enqueue only.  max_res = largest res in the table (it sizes the grid; the result
 * does not depend on it), at most 32768. */
#define NB_NOISE_SEEDED 3
int nb_noise_seeded_f32(const NbLayerDesc* layers_dev, int first_layer, int n_layers, int max_res, uint64_t seed, uint64_t offset,
                        const uint64_t* state_dev, int n, void* stream);

/* The first step of that arithmetic on its own: positions [n,2] int64 -> norm_pos_out [n,2] float32 = ((p mod R) / (R - 1)), the values
 * nb_noise_f32 derives internally (networks.py:371-374; same function, same bits).  For callers that hand NbNoiseSrc to the split-f16
 * convolutions: those evaluate the normalisation at the top of every tile, and from `positions` that is four 64-bit modulo operations
 * per lane and tile -- convert once per batch and pass `norm_pos`. */
int nb_norm_positions_f32(const int64_t* positions, int img_resolution, float* norm_pos_out, int n, void* stream);

/* Modulated 3x3 convolution + fused epilogue = SynthesisLayer.forward (networks.py:362-391) after
 * the affine:  y = clamp(lrelu(conv(x * s) * d + noise + bias, alpha) * gain, +-clamp)
 *   up = 1: cross-correlation, zero padding 1 (conv2d_resample.py:145-147)
 *   up = 2: stride-2 transposed convolution (true convolution, 2H+1) followed by the 4x4
 *           [1,3,3,1]x[1,3,3,1]/64 FIR with padding 1 and gain 4 (conv2d_resample.py:124-142)
 * The input is the channel-concatenation of x1 [n,c1,h,w] and (optionally) x2 [n,c2,h,w] -- the
 * geometry feature -- so no torch.cat copy is needed (networks_modified.py:218-219).
 * wpk is the packed, zero-padded weight [ceil8(c1+c2)][9][ceil32(c_out)] (tap = ky*3+kx) produced by
 * nb_pack_conv_weight.  x1, x2, wpk and y must be 16-byte aligned.
 * noise is [n or 1, h*up, w*up] with sample stride noise_stride_n (0 = shared), or NULL.
 * y is [n, c_out, h*up, w*up].  h and w must be powers of two >= 4. */
int nb_modconv3x3_f32(const float* x1, int c1, const float* x2, int c2, const float* wpk, const float* styles,
                      const float* dcoefs, const float* noise, int64_t noise_stride_n, const float* bias,
                      float* y, int n, int h, int w, int c_out, int up, float alpha, float gain, float clamp,
                      void* stream);

/* Name of the kernel template instance nb_modconv3x3_f32 launches for this problem shape (the name
 * rocprofv3 reports), so that a benchmark can attribute its per-launch timings to kernels. */
int nb_modconv3x3_variant(int n, int h, int w, int c_out, int up, char* buf, int buflen);

/* ---- split-f16 ("h3") fast path for the large conv1 layers (csrc/nb_modconv_up1_h3.hip, nb_modconv_up2_h3.hip, nb_pack_h2.hip) ----------------
 * Every fp32 operand is carried as hi + lo f16 halves and a product is three f16 MFMAs (xh*wh + xl*wh +
 * xh*wl, fp32 accumulate): fp32-grade results (5e-6 on pixels end to end) at ~5x the fp32-MFMA rate.
 * Activation format H2: _Float16 [n][ceil(c/8)][2 (hi,lo)][h][w][8], ALREADY multiplied by the consuming
 * layer's styles.  Weight format: produced by nb_pack_conv_weight_h3 (static, not modulated). */

/* fp32 NCHW (x1 [n,c1,hw] ++ x2 [n,c2,hw]) * scale[n, c1+c2] (or NULL) -> H2: v = x * scale is one fp32 multiply, hi = f16(v) (round to
 * nearest even), lo = f16(v - hi); channels >= c1 + c2 of the last group are written as zeros.
 * Input domain (the same for the f8 and f6 packers and the _part forms): x and scale finite, |x * scale| < 65520.  From 65520 on the
 * hi half is +-inf and the lo half -+inf, so hi + lo is NaN; nothing is clamped here.  The generator stays inside through the
 * activation clamp of 256 in front of every packer; the two producers that reach a packer without a clamp are the geometry encoder's
 * features (bounded by its folded weights on inputs in [-1, 1]) and the training path (nb_pack_h2_ranged_f32, whose power of two brings
 * max|x| max|scale| into (2^12, 2^14]). */
int nb_pack_h2_f32(const float* x1, int c1, const float* x2, int c2, const float* scale, void* out_h2, int n,
                   int hw, void* stream);

/* Host helper: W[c_out,c_in,3,3] fp32 -> hi/lo f16 [ceil(c_in/16)][3][3][2][2][ceil64(c_out)][8]
 * (bytes: ceil(c_in/16)*9*4*ceil64(c_out)*16). */
int nb_pack_conv_weight_h3(const float* w, int c_out, int c_in, void* out);
/* The same packing on the DEVICE (w and out are device pointers): one launch instead of a host loop -- for weights that
 * change every step (the training path evaluates its 3x3 convolutions on the split-f16 kernels, ops.TRAIN_SPLIT_F16).
 * co_align = 64 (modconv kernels) or 128 (encoder-type kernels); transpose_flip != 0: w is [c_in][c_out][3][3] and the packed
 * weight is its transpose with reversed taps (the kernel of the input-gradient convolution). */
int nb_pack_conv_weight_h3_dev(const float* w, int c_out, int c_in, int co_align, int transpose_flip, void* out, void* stream);

/* SynthesisLayer.forward with up = 1 (networks.py:362-391) on an H2 input:
 * y[n,c_out,h,w] (fp32 NCHW) = clamp(lrelu(conv3x3(x_h2, W) * dcoefs + noise + bias, alpha) * gain).
 * Needs w % 32 == 0 and h % 16 == 0 (the large layers); smaller layers use nb_modconv3x3_f32. */
int nb_modconv3x3_up1_h3(const void* x_h2, int c_in, const void* w_h3, const float* dcoefs, const float* noise,
                         int64_t noise_stride_n, const float* bias, float* y, int n, int h, int w, int c_out,
                         float alpha, float gain, float clamp, void* stream);

/* SynthesisLayer.forward with up = 2 (stride-2 transposed conv as 4 phases + fused 4x4 FIR, as in
 * nb_modconv3x3_f32) with split-f16 products: x_h2 is the H2 input [n, c_in, h, w] (already multiplied by this
 * layer's styles), y the fp32 NCHW output [n, c_out, 2h, 2w].  Needs w % 32 == 0. */
int nb_modconv3x3_up2_h3(const void* x_h2, int c_in, const void* w_h3, const float* dcoefs, const float* noise,
                         int64_t noise_stride_n, const float* bias, float* y, int n, int h, int w, int c_out,
                         float alpha, float gain, float clamp, void* stream);

/* nb_modconv3x3_f32 with up = 2 whose fused epilogue writes the result in H2 format, multiplied by
 * out_scale[n, c_out] (the styles of the conv1 layer that consumes it; NULL = 1), instead of fp32 NCHW. */
int nb_modconv3x3_up2_f32_h2(const float* x1, int c1, const float* x2, int c2, const float* wpk,
                             const float* styles, const float* dcoefs, const float* noise,
                             int64_t noise_stride_n, const float* bias, const float* out_scale, void* y_h2,
                             int n, int h, int w, int c_out, float alpha, float gain, float clamp, void* stream);

/* ToRGBColorTriadLayer.forward (networks.py:451-485) after its affine, on x [n,c,hw]:
 *   logits_o = clamp(sum_c x_c * styles[n,c] * w[o,c] + bias[o]);  uvs = softmax_o(logits)
 *   img[n,ch] = sum_k uvs_k * colors[n,ch,k]            (colors = tanh(affine[:, :9] + color_bias))
 * plus, optionally, the paint engine's compositing (forger/ui/brush.py:763-792):
 *   rgba[:3] = sum_k uvs_k * col01[n,:,k], rgba[3] = u+v ('clear', render_mode 0) or 1 ('full', 1)
 *   with col01 = user_colors (where not NaN) else (colors+1)/2; if sfactor [n] is given, (u,v,s) are first remapped
 *   per StyleUVSMapper._map_style_s (forger/ui/mapper.py:52-72; brush.py:773-774): s' = min(sfactor*s, 1),
 *   (u',v') = (u,v) * (1-s')/(u+v) (0 where 1-s' <= 1e-6) -- only in the RGBA outputs; rgba_f32 is [n,4,hw];
 *   rgba_u8 = trunc(clip(rgba*255, 0, 255)) is [n,hw,4] bytes (HWC, as brush.py:377 hands it out).
 * colors_raw is the [n, c_aff] affine output whose first 9 entries are the un-biased color scalars.
 * Any of logits / uvs / img / colors_out / rgba_f32 / rgba_u8 may be NULL. */
int nb_torgb_triad_f32(const float* x, const float* styles, int styles_stride_n, const float* w, const float* bias,
                       const float* color_bias, float clamp, float* logits, float* uvs, float* img,
                       float* colors_out, const float* user_colors, const float* sfactor, int render_mode,
                       float* rgba_f32, uint8_t* rgba_u8, int n, int c, int hw, void* stream);

/* BlendedFeatures.blend (forger/train/stitching.py:24-25): y = alpha*F + (1-alpha)*x over
 * x [n,c,hw]; F is [nf,c,hw] and alpha [na,1,hw] with nf, na in {1, n} (broadcast). */
int nb_blend_f32(const float* features, int nf, const float* alpha, int na, const float* x, float* y, int n, int c,
                 int hw, void* stream);

/* ---- "f8" operand format of the split-f16 convolutions: the two correction products on one block-scaled fp8 MFMA per
 * tap pair (csrc/nb_modconv_up1_h3.hip).  Same containers as H2 / nb_pack_conv_weight_h3, but the (cg, lo) slots of a
 * 16-channel chunk hold fp8 e4m3 values: activations (cg 2k, lo) = fp8(xl*2^9), (cg 2k+1, lo) = fp8(x/4); weights
 * (cg 0, lo) = fp8(w), (cg 1, lo) = fp8((w - f16(w))*2^11).  c_in % 16 == 0.  End-to-end pixel error ~1e-4 (H2: 5e-6).
 * Activations: xl = v - f16(v) of v = x * scale; both planes are e4m3 (OCP e4m3fn, subnormals down to 2^-9, round to nearest even) of
 * the value clamped to +-448, the 16 bytes of a slot in channel order; a zero code keeps the sign of its value.  Domain as for
 * nb_pack_h2_f32; inside it the fp8(x/4) plane saturates from |v| = 1792 on and fp8(xl*2^9) from |xl| = 0.875 on (|v| >= 2048), while
 * the hi half stays exact: the corrections lose accuracy there, the leading product does not. */
int nb_pack_h2f8_f32(const float* x1, int c1, const float* x2, int c2, const float* scale, void* out, int n, int hw,
                     void* stream);
/* c % 16 == 0 channels into the 16-channel chunks starting at channel group cg0 (even) of an f8-format tensor */
int nb_pack_h2f8_part_f32(const float* x, int c, const float* scale, int scale_stride, void* out, int c8_total, int cg0,
                          int n, int hw, void* stream);

/* ---- "f6" operand format (round 5): the two correction products on one block-scaled fp6 (e2m3) MFMA per tap pair, at the f16
 * instruction's cycles.  Same containers; the two lo slots of a 16-channel chunk (32 bytes per pixel / per (c_out, tap)) hold 32
 * six-bit fields (24 bytes), the chunk's E8M0 scale byte and zeros: activations field 2i = e2m3(xl[ch(i)]*2^11/S), field 2i+1 =
 * e2m3(x[ch(i)]/S), S = 2^(exponent of the chunk's largest |x| - 2), byte = S; weights field 2i = e2m3(w[ch(i)]/Sw), field 2i+1 =
 * e2m3((w - f16(w))[ch(i)]*2^11/Sw), byte = Sw*2^-11; ch(i) = channels 0-3, 8-11, 4-7, 12-15 of the chunk.  c_in % 16 == 0.
 * Operand format number 2 of nb_modconv3x3_up1_h3_ex / nb_modconv3x3_up2_h3_ex (0 = H2, 1 = f8).  Replaces nothing in the reference
 * (its convolutions are cuDNN calls, torch_utils/ops/conv2d_gradfix.py:35-43); the math it serves is training/networks.py:30-88.
 * Activations: x above = v = x * scale, the scale byte is floor(log2 m) - 2 + 127 for m = the chunk's largest |v| (so m / S lies in
 * [4, 8) and (7.5 S, 8 S) saturates), e2m3 rounds to nearest even and a zero code keeps the sign of its value; the 32 fields are a
 * little-endian 6-bit stream: bytes 0-15 in slot (cg 2k, lo), bytes 16-23, the scale byte and seven zero bytes in slot (cg 2k+1, lo).
 * An all-zero chunk has scale byte 0 and zero fields: 32 zero bytes (a -0.0 in it leaves the sign bit in its x field).  Domain as for
 * nb_pack_h2_f32, and m >= 2^-100 for a chunk that is not all zero. */
int nb_pack_h2f6_f32(const float* x1, int c1, const float* x2, int c2, const float* scale, void* out, int n, int hw,
                     void* stream);
/* c % 16 == 0 channels into the 16-channel chunks starting at channel group cg0 (even) of an f6-format tensor */
int nb_pack_h2f6_part_f32(const float* x, int c, const float* scale, int scale_stride, void* out, int c8_total, int cg0,
                          int n, int hw, void* stream);

/* Arguments of the triad ToRGB epilogue when it is fused into the last conv (same meaning as the parameters of
 * nb_torgb_triad_f32; any output pointer may be NULL). */
struct NbTorgbArgs {
    const float* styles;      /* [n, styles_stride_n]: 9 color scalars then c styles (affine output) */
    const float* w;           /* [3, c] */
    const float* bias;        /* [3] */
    const float* color_bias;  /* [9] */
    float* logits; float* uvs; float* img; float* colors_out;
    const float* user_colors; /* [n,3,3] or NULL */
    const float* sfactor;     /* [n] or NULL */
    float* rgba_f32; uint8_t* rgba_u8;
    int styles_stride_n, render_mode;
    float clamp;
};

/* Last SynthesisLayer (up = 1) + ToRGBColorTriadLayer + compositing in one launch: nb_modconv3x3_up1_h3 followed by
 * nb_torgb_triad_f32 on the tile while it is still in LDS (c_out <= 128).  y (the fp32 activations) may be NULL:
 * nothing but ToRGB reads them unless a caller taps the features. */
int nb_modconv3x3_up1_h3_torgb(const void* x_h2, int c_in, const void* w_h3, const float* dcoefs, const float* noise,
                               int64_t noise_stride_n, const float* bias, float* y, int n, int h, int w, int c_out,
                               float alpha, float gain, float clamp, const struct NbTorgbArgs* t, void* stream);

/* Constant noise computed INSIDE the split-f16 convolutions instead of being read from a [n, H, W] tensor that
 * nb_noise_f32 wrote (networks.py:371-382; the position-shifted bilinear sample of a <= 256 x 256 constant is four
 * L2-resident loads and a dozen FMAs per output pixel -- cheaper than writing and re-reading 22 MB per batch of 32).
 * Pass noise_stride_n = NB_NOISE_IN_KERNEL and, as `noise`, a HOST pointer to this struct (copied at launch) to
 * nb_modconv3x3_up1_h3_ex / nb_modconv3x3_up2_h3_ex.  Same expressions, same order as nb_noise_f32: bit-identical. */
#define NB_NOISE_IN_KERNEL (-1)
struct NbNoiseSrc {
    const float* noise_const_t;   /* [res, res]: the layer's noise_const TRANSPOSED (the sampling grid transposes: SURVEY note C) */
    const float* noise_lin;       /* [res]: noise_grid[0, :, 0, 0] */
    const float* noise_strength;  /* [1] */
    const float* norm_pos;        /* [n, 2] normalised positions, or NULL */
    const int64_t* positions;     /* [n, 2] integer (y, x) positions (normalised in-kernel like nb_noise_f32), or NULL; exactly one */
    int res;                      /* resolution of the layer's OUTPUT */
    int img_resolution;           /* R of (positions % R) / (R - 1) */
};

/* General forms of the two split-f16 convolutions.  in_fmt / out_fmt: 0 = H2 (hi/lo f16), 1 = "f8" (hi f16 + fp8
 * correction operands, above); the weights must be packed for in_fmt (nb_pack_conv_weight_h3 or the f8 layout).
 * in_fmt 2 = "f6" (round-5 experiment: fp6 corrections, own weight layout).  in_fmt 3 (round 6) = f8 operands and weights with the
 * correction products SKIPPED where the launch runs on the large throughput kernels (ping-pong up=1 loop, 12-row up=2 kernel;
 * elsewhere it is in_fmt 1): a plain single-f16 evaluation, 1.5e-3 ... 3e-3 from fp32 end to end -- the reference's own shipped arithmetic for
 * blocks >= 32^2 (training/networks.py:634-638), outside this build's 1e-3 parity budget; Generator(conv_mode="f16"), a timing
 * data point, not a parity mode.
 * Exactly one destination: y_f32 (fp32 NCHW; out_fmt ignored), y_h2 (the consumer's input tensor [n, c_next, ...] in
 * out_fmt, multiplied by next_styles), or -- up1 only, t != NULL -- the fused ToRGB outputs (y_f32 optional). */
int nb_modconv3x3_up1_h3_ex(const void* x, int c_in, const void* wts, const float* dcoefs, const float* noise,
                            int64_t noise_stride_n, const float* bias, float* y_f32, void* y_h2, const float* next_styles,
                            int next_stride, int c_next, const struct NbTorgbArgs* t, int in_fmt, int out_fmt, int n, int h,
                            int w, int c_out, float alpha, float gain, float clamp, void* stream);
int nb_modconv3x3_up2_h3_ex(const void* x, int c_in, const void* wts, const float* dcoefs, const float* noise,
                            int64_t noise_stride_n, const float* bias, float* y_f32, void* y_h2, const float* next_styles,
                            int next_stride, int c_next, int in_fmt, int out_fmt, int n, int h, int w, int c_out,
                            float alpha, float gain, float clamp, void* stream);

/* Name of the kernel nb_modconv3x3_up2_h3 / _ex launches for this problem shape (the name rocprofv3 reports: the round-3 8-wave
 * kernel in one of its tile forms, or the software-pipelined 8-wave kernel of csrc/nb_modconv_up2v.hip), so that a benchmark can
 * attribute its per-launch timings to kernels.  in_fmt as in _ex. */
int nb_modconv3x3_up2_h3_variant(int in_fmt, int c_in, int c_out, int n, int h, int w, char* buf, int buflen);

/* The same layer for SMALL images (csrc/nb_modconv_small.hip; the <= 64x64 conv1 layers): split-f16 products on
 * 32 c_out x 32 position tiles with K split over the 4 waves of a workgroup, fp32 NCHW in and out, the per-sample styles
 * applied to the activations while they are split into hi/lo f16 on their way into LDS.  Replaces nb_modconv3x3_f32
 * (up = 1) where the fp32 matrix rate or the launch latency of few, long workgroups dominates: h, w powers of two >= 4
 * (4x4 images are processed two samples per tile), c_in <= 512.  w_h3 = the nb_pack_conv_weight_h3 format. */
int nb_modconv3x3_up1_small_h3(const float* x, int c_in, const void* w_h3, const float* styles, const float* dcoefs,
                               const float* noise, int64_t noise_stride_n, const float* bias, float* y, int n, int h,
                               int w, int c_out, float alpha, float gain, float clamp, void* stream);

/* up = 2 (conv2d_resample.py:124-142: stride-2 transposed conv + 4x4 FIR, pad 1, gain 4) for small images through the same
 * kernel: per output phase (py, px) the composite is a 3x3 correlation of the input grid with an effective kernel
 * Keff[py,px] = W folded with the FIR (static, no styles), so w_h3_phases = the four nb_pack_conv_weight_h3(Keff[2 py + px])
 * images back to back and the kernel runs the phases as grid.z.  (x1 ++ x2) = concatenated input, c1, c2 % 16 == 0;
 * h, w = INPUT size; y [n, c_out, 2h, 2w]; noise [.., 2h, 2w]. */
int nb_modconv3x3_up2_small_h3(const float* x1, int c1, const float* x2, int c2, const void* w_h3_phases, const float* styles,
                               const float* dcoefs, const float* noise, int64_t noise_stride_n, const float* bias, float* y,
                               int n, int h, int w, int c_out, float alpha, float gain, float clamp, void* stream);

/* The two split-f16 convolutions with the output written straight into the CONSUMER's H2 input tensor
 * y_h2 = H2 [n, c_next, h_out, w_out] (channel groups 0 .. c_out/8-1; c_out % 8 == 0), already multiplied by the
 * consumer's styles next_styles[n*next_stride + c] -- the fused form of SynthesisLayer.forward followed by the next
 * layer's `x * styles` (networks.py:67, 362-391).  Removes the separate nb_pack_h2_f32 pass between two such layers. */
int nb_modconv3x3_up1_h3_h2(const void* x_h2, int c_in, const void* w_h3, const float* dcoefs, const float* noise,
                            int64_t noise_stride_n, const float* bias, const float* next_styles, int next_stride,
                            void* y_h2, int c_next, int n, int h, int w, int c_out, float alpha, float gain, float clamp,
                            void* stream);
int nb_modconv3x3_up2_h3_h2(const void* x_h2, int c_in, const void* w_h3, const float* dcoefs, const float* noise,
                            int64_t noise_stride_n, const float* bias, const float* next_styles, int next_stride,
                            void* y_h2, int c_next, int n, int h, int w, int c_out, float alpha, float gain, float clamp,
                            void* stream);

/* fp32 NCHW x [n,c,hw] * scale[n*scale_stride + ch] (or NULL) -> channel groups cg0.. of an H2 tensor with c8_total
 * groups: the geometry features concatenated behind a producer that wrote its groups itself (NM:218-219). */
int nb_pack_h2_part_f32(const float* x, int c, const float* scale, int scale_stride, void* out_h2, int c8_total, int cg0,
                        int n, int hw, void* stream);

/* ---- canvas side of the painting engine (SURVEY 8 rows e / f2) ---------------------------------------------
 * Cells: the canvas is cut into NB_CELL_H x NB_CELL_W pixel cells (row-major, ceil(w/NB_CELL_W) per row);
 * cell_off [ncells+1] / cell_tiles is a CSR list of the tiles whose rectangle touches each cell, in ascending
 * tile order (= the reference's sequential paint order).  All pointers are device pointers. */
#define NB_CELL_H 4
#define NB_CELL_W 64

/* Geometry tiles for the encoder: out[t,0,y,x] = 1 - (255 - geom[ty+y, tx+x]) / 255  (outside the image: 1), i.e.
 * forger/viz/paint_image_main.py:162 (`255 - geom[y:y+P, x:x+P]`) followed by GanPaintEngine.prepare_geom_input
 * (forger/ui/brush.py:672-681).  geom is [gh,gw] uint8 (255 = background), tile_yx [t,2] int32. */
int nb_geom_tiles_f32(const uint8_t* geom, int gh, int gw, const int32_t* tile_yx, int t, int r, float* out,
                      void* stream);

/* Feature-canvas blending for a SEQUENCE of full tiles in one launch.  Replaces, for tiles 0..t-1 in order,
 * PaintingHelper._get_blended_features (forger/ui/brush.py:190-227) + BlendedFeatures.blend (forger/train/
 * stitching.py:24-25, applied in networks_modified.py:176-181) + FeatureCanvas.set_features (brush.py:82-92):
 *   upd = alpha0 > 0.99 | (mask & alpha0 > 0), cleared inside the `crop` border;  a = 1 - (mask ? alpha0 : 1);
 *   tiles[t] = a * canvas + (1 - a) * tiles[t];  canvas[upd] = tiles[t][upd];  mask |= upd.
 * tiles [t,c,hw,hw] holds the block output before blending on entry and the blended features on return;
 * tile_yx [t,2] are tile origins on the feature canvas; alpha0 [hw,hw] is generate_dirty_area_alpha
 * (brush.py:159-187) for a full tile; canvas [c,hc,wc] / mask_in / mask_out [hc,wc] are the FeatureCanvas state
 * (mask_out must not alias mask_in).  Cells are taken over the feature canvas. */
int nb_canvas_replay_f32(float* tiles, int t, int c, int hw, const int32_t* tile_yx, const float* alpha0, int crop,
                         float* canvas, const uint8_t* mask_in, uint8_t* mask_out, int hc, int wc,
                         const int32_t* cell_off, const int32_t* cell_tiles, void* stream);

/* The same restricted to the cells [cell_y0, cell_y0 + cells_y) x [cell_x0, cell_x0 + cells_x) (cell = NB_CELL_H x NB_CELL_W
 * canvas pixels, the granularity of cell_off): for the interactive stroke, which replays ONE tile on a large canvas.
 * mask_out is only written inside the box - the caller starts it as a copy of mask_in. */
int nb_canvas_replay_box_f32(float* tiles, int t, int c, int hw, const int32_t* tile_yx, const float* alpha0,
                             int crop, float* canvas, const uint8_t* mask_in, uint8_t* mask_out, int hc, int wc,
                             const int32_t* cell_off, const int32_t* cell_tiles, int cell_x0, int cell_y0,
                             int cells_x, int cells_y, void* stream);

/* The replay over tile PIECES, for the multi-GPU halo exchange ("P2P halo send/recv of only the overlapped
 * strips"): a rank replays its own tiles together with the strips of earlier foreign tiles that overlap them.  A piece is
 * a rectangle [ly0, ly0+h) x [lx0, lx0+w) of one tile, sitting at (cy, cx) on the feature canvas, with its values at
 * data[ch * cstride + row * rstride + col] (a full own tile: h = w = hw, rstride = hw, cstride = hw*hw; a received strip:
 * a compact buffer).  Pieces of one tile must be disjoint; ascending piece index = paint order (cell_pieces lists piece
 * indices).  Same per-pixel arithmetic as nb_canvas_replay_f32; only the cells of the given box run and mask_out is only
 * written there (start it as a copy of mask_in). */
typedef struct NbTilePiece {
    uint64_t data;               /* device pointer (float*) */
    int32_t cstride, rstride;    /* in floats */
    int32_t cy, cx, h, w;        /* piece rectangle on the feature canvas */
    int32_t ly0, lx0;            /* its origin inside the tile (alpha template / crop border lookup) */
} NbTilePiece;
int nb_canvas_replay_pieces_f32(const NbTilePiece* pieces, int n, int c, int hw, const float* alpha0, int crop,
                                float* canvas, const uint8_t* mask_in, uint8_t* mask_out, int hc, int wc,
                                const int32_t* cell_off, const int32_t* cell_pieces, int cell_x0, int cell_y0,
                                int cells_x, int cells_y, void* stream);

/* Paste RGBA8 tiles [t,r,r,4] into canvas [h,w,4]: the interior [crop, r-crop)^2 of tile i lands at
 * dst_yx[i] + crop (brush.py:369-374 crop + out_meta, paint_image_main.py:173-177 paste); later tiles
 * overwrite earlier ones.  Cells are taken over the RGBA canvas from the interior rectangles. */
int nb_paste_tiles_u8(const uint8_t* tiles, int t, int r, const int32_t* dst_yx, int crop, uint8_t* canvas, int h, int w,
                      const int32_t* cell_off, const int32_t* cell_tiles, void* stream);

/* The alpha0 template of nb_canvas_replay_*_f32 written on the device: PaintingHelper.generate_dirty_area_alpha (forger/ui/brush.py:159-187)
 * for a dirty area spanning the whole tile of `width` pixels: 1 inside the square inset by margin + crop, a linear fall-off of width
 * `margin` outside it (distance to the nearest edge; to the nearest corner in the corner regions), 0 beyond.  alpha0_dev [width, width]
 * fp32.  fp32 throughout with correctly rounded sqrt and division, in the reference's expression order: bit for bit what the numpy
 * of the reference computes.  margin <= 0, or margin + crop leaving no interior: NB_EINVAL.  (The engine passes the blend margin 16 and
 * the tile's crop margin, both divided by the blending level's down factor: brush.py:190-227.) */
int nb_dirty_area_alpha_f32(float* alpha0_dev, int width, int margin, int crop, void* stream);

/* The cell lists above for a host without numpy (HOST ONLY: no HIP call, host pointers).  rects [t, 4] int32 (y0, x0, y1, x1),
 * end-exclusive, clipped to the h x w grid here; rectangles that miss the grid are dropped.  For the replay the rectangles are the
 * tiles' areas on the feature canvas (brush.py:253-258: the tile origin floored to the blending grid, divided by the down factor),
 * for the paste the tiles' interiors.  nb_canvas_cells_count returns the number of list entries (>= 1: a list without entries is a
 * single 0, so that its device copy is never empty) or a negative NB_E* code; nb_canvas_build_cells fills cell_off
 * [ceil(h / NB_CELL_H) * ceil(w / NB_CELL_W) + 1] and cell_items [that count], every cell's rectangles in ascending order. */
int nb_canvas_cells_count(const int32_t* rects, int t, int h, int w);
int nb_canvas_build_cells(const int32_t* rects, int t, int h, int w, int32_t* cell_off, int32_t* cell_items);

/* ---- drawing preparation: from a decoded drawing to the padded geometry, the tile picks and the image on white ------------------
 * What forger/viz/paint_image_main.py does on the host before and after its tile loop.  The three device entries only enqueue on
 * `stream` (no allocation, no synchronisation, no read-back: they can be captured into a hipGraph); all pointers but those of
 * nb_stitching_grid are device pointers. */

/* _read_any_geo (paint_image_main.py:30-57) with threshold_img (forger/util/img_proc.py:66-71: skimage's threshold_otsu, one bin per
 * integer value) on a decoded drawing, written straight into the padded geometry of paint_image_main.py:58-61 and
 * generate_stitching_crops (forger/viz/style_transfer.py:24-31).  img [h,w,channels] uint8 (HWC), channels 1 (gray), 3 (RGB) or
 * 4 (RGBA); out [out_h,out_w] uint8: the thresholded drawing (255 = background, 0 = stroke) at (off_y, off_x), 255 around it.
 *   gray (fp32)  the value | ((r + g) + b) / 3 | mean * alpha + 255 * (1 - alpha) with alpha = a / 255 -- separate, unfused multiply,
 *                subtract and add, correctly rounded divisions;
 *   stretch      subtract the global minimum if it is > 0, then scale by (float)(255.0 / (double)max) if 0 < max < 255; truncate to uint8;
 *   threshold    Otsu over the occupied value range in float64, cumulative sums in sequential order, first maximum of
 *                var12 = w1 * w2 * (m1 - m2)^2 (a constant image: its value);
 *   out          gray8 > threshold ? 255 : 0.
 * Byte for byte what the numpy code of the reference produces.  The passes recompute the gray value from img: no scratch the size of
 * the drawing.  ws: NB_GEOM_PREP_WS_BYTES of 4-byte aligned device scratch, cleared by the call itself, holding on completion as
 * uint32 words: [0] / [1] the bit patterns of the fp32 minimum / maximum gray value, [2] the threshold, [4..259] the histogram of
 * the stretched uint8 image (its counts sum to h * w).  Calls that share a ws must be ordered (one stream).
 * NB_EINVAL: a null pointer, another channel count, an image that does not fit into out at the offset, h * w >= 2^31. */
#define NB_GEOM_PREP_WS_BYTES 1040
int nb_geom_prepare_u8(const uint8_t* img, int h, int w, int channels, uint8_t* out, int out_h, int out_w, int off_y, int off_x,
                       void* ws, void* stream);

/* Stroke pixels per tile: counts[row * ncols + col] = number of pixels equal to 0 in the r x r window of geom [gh,gw] at
 * (row * stride, col * stride); pixels outside the image are background.  The `np.sum(padded[...] < 0.001)` of
 * generate_stitching_crops (style_transfer.py:15-48) for every tile in one launch: with a mode other than "all" the host copies
 * the nrows * ncols counts back and keeps, in row-major order, the tiles with a count above 10. */
int nb_tile_stroke_counts_u8(const uint8_t* geom, int gh, int gw, int r, int stride, int nrows, int ncols, int32_t* counts,
                             void* stream);

/* The crop and `--on_white` of paint_image_main.py:179-183 in one pass: canvas [ch,cw,4] RGBA8 (4-byte aligned), out [h,w,3] =
 * trunc(clip(rgb * a + 255 * (1 - a), 0, 255)) of the window at (y0, x0), a = alpha / 255 correctly rounded, unfused fp32. */
int nb_composite_on_white_u8(const uint8_t* canvas, int ch, int cw, int y0, int x0, int h, int w, uint8_t* out, void* stream);

/* The tile grid of generate_stitching_crops (style_transfer.py:15-32) for an [h,w] image (HOST ONLY: no HIP call, works without a
 * GPU): stride = patch_width - 2 * overlap_margin, nrows = h / stride + 1, ncols = w / stride + 1, tile (row, col) at
 * (row * stride, col * stride), padded size = rows-or-cols * stride + patch_width.  paint_image_main pads the drawing by its crop
 * margin m first (h + m, w + m here, offsets (m, m) for nb_geom_prepare_u8) and tiles with overlap_margin = 2 m.
 * NB_EINVAL when patch_width - 2 * overlap_margin <= 0. */
int nb_stitching_grid(int h, int w, int patch_width, int overlap_margin, int* nrows, int* ncols, int* stride, int* padded_h,
                      int* padded_w);

/* ---- vector strokes: polylines and splines rasterised into the geometry on the device (csrc/nb_strokes.hip) -----------------------
 * The route from stroke points to the padded geometry without a raster on the host: what drawing the strokes into an image, then
 * _read_any_geo and the padding of forger/viz/paint_image_main.py:30-61 would produce, with nothing the size of the canvas uploaded.
 * Coordinates: drawing coordinates are (x, y) in pixels, pixel (row y, column x) has its centre at exactly (x, y), and pixel (Y, X)
 * of an output buffer is the drawing position (X - off_x, Y - off_y).  A segment row is NB_SEG_PITCH = 8 floats (32 bytes):
 * x0, y0, x1, y1, r and three reserved floats (ignored by the rasteriser, written as zeros by the flattener).  Both device entries
 * only enqueue on `stream` (no allocation, no synchronisation, no read-back: they can be captured into a hipGraph), validate on the
 * host before any launch and never dereference their pointers on the host. */
#define NB_SEG_PITCH 8

/* out [out_h,out_w] uint8 geometry (255 = background, 0 = stroke; any alignment, any width): a pixel is stroke iff the distance from
 * its centre to the closed segment (x0,y0)-(x1,y1) is <= r for some of the n_segs rows of segs (device fp32, 16-byte aligned).  A row
 * with equal end points is a disc; a row in which one of the five values is not finite, or r < 0, draws nothing.  clear = 1: every
 * byte of out is written (255 where no stroke); clear = 0: only stroke pixels are written, as 0, and every other byte keeps its
 * value (more strokes on a prepared drawing).  n_segs = 0 is legal (segs may then be NULL): with clear = 1 it fills 255.  The result
 * is a union: independent of the order of the rows, bit-identical from run to run.  Arithmetic: fp32, unfused, distances relative to
 * the segment's first point (differences first): within ~1e-4 px of the exact distance on canvases up to 8192.
 * Cost: one workgroup per 64 x 64 pixels of out, each reading all rows (ceil(out_h / 64) * ceil(out_w / 64) * n_segs box tests).
 * NB_EINVAL: a null pointer, n_segs < 0, non-positive sizes, out_h * out_w >= 2^31, clear other than 0 / 1, unaligned segs. */
int nb_raster_segments_u8(const float* segs, int n_segs, uint8_t* out, int out_h, int out_w, int off_y, int off_x, int clear,
                          void* stream);

/* Centripetal Catmull-Rom strokes cut into segment rows: the curve of forger/core/curve.py (knots ts = cumsum(|dP|^alpha), lines
 * 24-37; a point by the pyramid A1..A3 -> B1, B2 -> C of sample_t_one, lines 50-85).  ctrl [n_points_total][3] device fp32 (x, y, r
 * per control point), stroke_off [n_strokes + 1] device int32 offsets into ctrl (stroke_off[0] = 0, stroke_off[n_strokes] =
 * n_points_total, every stroke >= 4 points).  Like the reference's, the curve of a stroke with P points runs from its control point 1
 * to its control point P - 2: P - 3 spans, each cut into subdiv pieces uniform in t.  Every sample point is evaluated once and
 * written as the end of one segment and the start of the next (bit-equal: watertight polylines); a segment's radius is its span's two
 * control radii interpolated linearly at the piece's mid t.  Stroke s starts at row (stroke_off[s] - 3 s) * subdiv of segs (closed
 * form: no scan, no atomics); nb_spline_segment_count rows are written in all.  A span next to a repeated control point has a zero
 * knot interval and yields non-finite rows, which nb_raster_segments_u8 does not draw (drop consecutive duplicates beforehand).
 * stroke_off is read on the device only: the capacity check uses the totals passed here, and a table that disagrees with them (an
 * offset outside 0..n_points_total, a stroke of fewer than 4 points) makes the kernel skip that stroke, never write outside segs.
 * NB_EINVAL: a null pointer, n_strokes < 1, subdiv < 1, n_points_total < 4 * n_strokes, alpha outside [0, 1], seg_capacity (rows)
 * below the count, unaligned segs. */
int nb_spline_flatten_f32(const float* ctrl, const int32_t* stroke_off, int n_points_total, int n_strokes, int subdiv, float alpha,
                          float* segs, int seg_capacity, void* stream);

/* (n_points_total - 3 * n_strokes) * subdiv: the segment rows nb_spline_flatten_f32 writes (HOST ONLY: no HIP call, works without a
 * GPU).  NB_EINVAL (negative) for n_strokes < 0, subdiv < 1 or n_points_total < 4 * n_strokes. */
long long nb_spline_segment_count(int n_points_total, int n_strokes, int subdiv);

/* ---- synthetic drawings: seeded random spline patches, rasterised K at a time (csrc/nb_drawings.hip) -----------------------------
 * What scripts/create_splines.py of the reference makes on the host, one image per process-pool task: random centripetal
 * Catmull-Rom control points (create_splines.py:35-39, forger/core/curve.py:98-116 sample_control_pts2), a thickness from a Gaussian
 * mixture or an integer range (forger/util/spline_dist.py:37-96) or a fixed radius (--use_radii, create_splines.py:49-52), the curve
 * drawn and dilated (create_splines.py:47-59).  Here: counts -> control points -> nb_spline_flatten_f32 -> one batch raster.
 * Departures, all stated: (1) the draws are a pure function of (seed, drawing, draw index) instead of the process-global `random`
 * and `np.random` streams; (2) the drawing is the capsule union of nb_raster_segments_u8, not a sampled curve dilated by a disc;
 * (3) sample_control_pts2 marks the TRANSPOSED cell as used (curve.py:110, quadrants[idx[1], idx[0]]), so it can repeat a cell while
 * others stay free; that is not reproduced: cells are used without replacement; (4) the thickness loop `while res < -0.5`
 * (spline_dist.py:75-76) is bounded to eight tries.
 *
 * The draws.  For drawing k of a call, s = offset + k (uint64, wraps), and
 *     P(j) = Philox4x32-10(counter = (j, 0x53504C4E, lo32(s), hi32(s)), key = (lo32(seed), hi32(seed)))  -> (x0, x1, x2, x3)
 * with the constants of nb_noise_seeded_f32; u(x) = (x >> 8) * 2^-24 (exact in fp32).  So drawing k at offset o is drawing 0 at
 * offset o + k, at any batch size.
 *   P(0):        npts = pts_min + x0 mod (pts_max - pts_min + 1).  Mixture component c = the first with u(x1) < cdf[c].  Integer-range
 *                thickness: radius = rmin + x2 mod (rmax - rmin + 1).
 *   P(1 + i), i = 0..7: Gaussian thickness tries.  z = the even normal of pair(x0, x1) as nb_noise_seeded_f32 defines it;
 *                v = center[c] + sigma[c] * z (one fp32 multiply, one add); the first v >= -0.5 is taken, radius = rintf(v); none
 *                accepted: radius 0.
 *   P(16 + i), i < npts: control point i.  NB_SPLINE_CELLS, i < 16: the free cell number x0 mod (16 - i) of the 4 x 4 grid, free
 *                cells counted in ascending index, cx = cell mod 4, cy = cell div 4, X = (cx + u(x1)) * (r / 4), Y = (cy + u(x2)) *
 *                (r / 4); i >= 16: X = (u(x1) * 1.1f - 0.05f) * r, Y likewise from x2.  NB_SPLINE_UNIFORM (rand * 2.2 - 1 of
 *                create_splines.py:39 in pixels): X = (u(x1) * 1.1f) * r, Y from x2.
 *   The row is (X, Y, r_eff), r_eff = radius for radius >= 2 and 0.5 below (the reference leaves its one-pixel curve undilated
 *   below 2, create_splines.py:58).  Coordinates carry at most NB_SYNTH_COORD_ROUNDINGS fp32 roundings, each within one ulp(1.1 r).
 * The curve of a drawing runs from its control point 1 to npts - 2 (draw_spline_custom; nb_spline_flatten_f32 does the same). */
#define NB_SPLINE_UNIFORM 0
#define NB_SPLINE_CELLS 1
#define NB_THICK_FIXED 0
#define NB_THICK_RANGE 1
#define NB_THICK_MIXTURE 2
#define NB_SYNTH_MAX_POINTS 64
#define NB_SYNTH_MAX_MIX 4
#define NB_SYNTH_COORD_ROUNDINGS 3
typedef struct NbSplineSpec {
    int32_t pts_min, pts_max;     /* 4 <= pts_min <= pts_max <= NB_SYNTH_MAX_POINTS (reference: 4..15) */
    int32_t mode;                 /* NB_SPLINE_UNIFORM | NB_SPLINE_CELLS (--smart_sampling) */
    int32_t thick_mode;           /* NB_THICK_FIXED | NB_THICK_RANGE | NB_THICK_MIXTURE */
    float radius;                 /* NB_THICK_FIXED: the radius in pixels, >= 0 */
    int32_t rmin, rmax;           /* NB_THICK_RANGE: 0 <= rmin <= rmax (reference: 1..30) */
    int32_t n_mix;                /* NB_THICK_MIXTURE: 1..NB_SYNTH_MAX_MIX components */
    float center[4], sigma[4];    /* (reference: centres 6, 10, sigmas 2, 3, for 256-pixel patches) */
    float cdf[4];                 /* normalised cumulative weights (reference: 6 : 10), non-decreasing, cdf[n_mix - 1] = 1 */
} NbSplineSpec;

/* npts[k] control points of drawings offset .. offset + k - 1 (HOST ONLY: no HIP call, works without a GPU; pure integer
 * arithmetic).  From it the caller builds stroke_off [k + 1] and the totals of nb_synth_spline_ctrl_f32 and nb_spline_flatten_f32
 * with no device read-back.  NB_EINVAL: a null pointer, k < 0, a spec outside the ranges stated at NbSplineSpec. */
int nb_synth_spline_counts(const NbSplineSpec* spec, uint64_t seed, uint64_t offset, int k, int32_t* npts);

/* ctrl [n_points_total][3] device fp32: rows stroke_off[d] .. stroke_off[d + 1] are the control points (X, Y, r_eff) of drawing d
 * of side r, d < k.  spec is a host struct, passed by value to the kernel; stroke_off [k + 1] is device int32 and read on the device
 * only.  One lane per drawing (the cell choice is sequential).  A drawing whose stroke_off entries disagree with its count, or
 * reach outside 0..n_points_total, is skipped: nothing outside ctrl is ever written.  Enqueue only.  NB_EINVAL: a null pointer, a
 * bad spec, k < 1, r outside 1..2^20, n_points_total outside pts_min * k .. pts_max * k. */
int nb_synth_spline_ctrl_f32(const NbSplineSpec* spec, uint64_t seed, uint64_t offset, int k, int r, const int32_t* stroke_off,
                             float* ctrl, int n_points_total, void* stream);

/* out [k,h,w] uint8 (any alignment, any size): drawing i is rows seg_off[i] .. seg_off[i + 1] of segs (NB_SEG_PITCH floats each, device
 * fp32, 16-byte aligned; seg_off [k + 1] device int32), rasterised under the contract of nb_raster_segments_u8 with clear = 1: every
 * byte is written, a drawing with an empty range is all 255, rows with a non-finite value or r < 0 draw nothing, and the bytes are
 * IDENTICAL to that entry's on the same rows (the per-cell code is one function).  A drawing's rows darken that drawing only:
 * curves that leave the patch are clipped at its edges.  A range outside 0..n_segs_total, or a decreasing one, draws nothing and
 * reads nothing.  This replaces the draw and the dilation of create_splines.py:47-59 for K images at once.  One 256-thread workgroup
 * per 64 x 64 cell of one drawing (grid = k * cells).  Enqueue only.  NB_EINVAL: a null pointer, n_segs_total < 0, k < 1,
 * non-positive sizes, h * w >= 2^31, k * cells >= 2^31, unaligned segs. */
int nb_raster_batch_u8(const float* segs, const int32_t* seg_off, int n_segs_total, int k, uint8_t* out, int h, int w, int off_y,
                       int off_x, void* stream);

/* ---- compositing for a paint session: tiles over a canvas, a reduced view of a window (csrc/nb_compose.hip) ----------------------
 * What the reference leaves to its browser client -- the patches of a stroke written into a foreground layer with putImageData
 * (forger/ui/js/main_controller.js:776) and that layer drawn over the background canvas when the stroke ends
 * (main_controller.js:131-141) -- on a canvas that stays on the device.  RGBA8 with straight (unpremultiplied) alpha; all of it is
 * integer arithmetic with floor division, so a restatement in integers matches byte for byte (painting.over_tiles_numpy,
 * painting.canvas_view_numpy).  Both entries only enqueue on `stream` (no allocation, no synchronisation: they can be captured into
 * a hipGraph) and validate on the host before any launch; all pointers are device pointers, canvases and tiles 4-byte aligned.  A
 * canvas that is 16-byte aligned with a width that is a multiple of 4 pixels is read and written in 16-byte vectors. */

/* RGBA8 tiles [t,r,r,4] composited onto canvas [h,w,4] in place.  Tile selection is that of nb_paste_tiles_u8: the source of a
 * canvas pixel is the LAST tile i whose interior [crop, r-crop)^2, placed at dst_yx[i] + crop, covers it (origins may be negative,
 * tiles may hang over the canvas); cell_off / cell_tiles are the cell lists of the interior rectangles over the canvas.  Only the
 * cells [cell_y0, cell_y0 + cells_y) x [cell_x0, cell_x0 + cells_x) run: a pixel that no interior covers keeps its four bytes, and
 * so does every pixel outside that box.  With source (cs, as), destination (cd, ad) and opacity in 0..255:
 *   ae = (as * opacity + 127) / 255
 *   mode 0 (paint, source-over):   t = ad * (255 - ae);  den = ae * 255 + t;
 *                                  alpha = (den + 127) / 255;  colour = den > 0 ? (cs * ae * 255 + cd * t + den / 2) / den : 0
 *   mode 1 (erase, destination-out by the rendered stroke's alpha):
 *                                  alpha = (ad * (255 - ae) + 127) / 255;  colour = cd
 * The colour of mode 0 is the integer nearest to the exact quotient, ties rounded up; a transparent destination yields (cs, ae), a
 * transparent source leaves the alpha as it was; the largest intermediate is 16 613 887.
 * NB_EINVAL: a null pointer, non-positive sizes, 2 * crop >= r, a mode other than 0 / 1, an opacity outside 0..255, a cell box that
 * is empty or leaves the canvas's cells, h * w >= 2^31, unaligned tiles or canvas. */
int nb_over_tiles_u8(const uint8_t* tiles, int t, int r, const int32_t* dst_yx, int crop, uint8_t* canvas, int h, int w,
                     const int32_t* cell_off, const int32_t* cell_tiles, int cell_x0, int cell_y0, int cells_x, int cells_y,
                     int mode, int opacity, void* stream);

/* The window [y0, y0 + h) x [x0, x0 + w) of canvas [ch,cw,4] reduced by the integer factor k in 1..16: out is
 * [ceil(h / k), ceil(w / k), 4] RGBA8 (4-byte aligned), or [.., 3] RGB8 over white with on_white = 1.  Every k x k block is clipped to
 * the window and n is the number of pixels left in it; with SA = sum of a and SC = sum of c * a (per channel) over the block:
 *   on_white 0:   alpha = (SA + n / 2) / n;  colour = SA > 0 ? (SC + SA / 2) / SA : 0
 *   on_white 1:   colour = (SC + 255 * (255 * n - SA) + (255 * n) / 2) / (255 * n)
 * (alpha-weighted means, rounded half up; the sums stay below 2^25 at k = 16).  This is the PREVIEW path -- a large canvas reduced
 * before it crosses PCIe; at k = 1 with on_white = 1 it rounds to nearest where nb_composite_on_white_u8 truncates the reference's
 * fp32 expression, so the exported image keeps nb_composite_on_white_u8.
 * NB_EINVAL: a null pointer, non-positive sizes, k outside 1..16, on_white other than 0 / 1, a window that leaves the canvas,
 * ch * cw >= 2^31, an unaligned canvas (or RGBA out). */
int nb_canvas_view_u8(const uint8_t* canvas, int ch, int cw, int y0, int x0, int h, int w, int k, int on_white, uint8_t* out,
                      void* stream);

/* ---- masked selection: the k-th largest included value of every image (csrc/nb_select.hip) ---------------------------------------
 * What StyleUVSMapper calibrates on (forger/ui/mapper.py:132: `torch.topk(S[i][bmask[i]], k=15)[0].min()` per drawing), for a batch
 * of images in one launch.  Image i is the `count` floats at x + i * stride_n (stride_n >= count, so images never alias; a stride
 * lets one channel of an NCHW tensor be read in place) and uses mask (i % n_masks): `count` bytes at mask + (i % n_masks) * count,
 * non-zero = included.  n_masked[i] = the number of included elements.  kth[i] = the k-th largest included value in the order of
 * torch.topk(largest=True) on the CPU: every NaN ranks above +inf (a selected NaN comes back as the quiet NaN 0x7fc00000), -0 and +0
 * compare equal and the sign of a returned zero is unspecified.  Where n_masked[i] < k, kth[i] is a quiet NaN: the caller decides from
 * n_masked.  Exact (a radix select on the values' bits, integer arithmetic only) and bit-identical from run to run.  No workspace, no
 * allocation, no synchronisation: the entry only enqueues on `stream`.  x may start at any float; rows that are 16-byte aligned
 * somewhere are read in 16-byte vectors from there on.  n == 0: NB_OK without a launch.
 * NB_EINVAL (before any HIP call): a null pointer, k < 1, count < 1, n_masks < 1, n < 0, stride_n < count, x / kth / n_masked not
 * 4-byte aligned. */
int nb_masked_kth_largest_f32(const float* x, long long stride_n, const uint8_t* mask, int n_masks, int count, int k, int n,
                              float* kth, int32_t* n_masked, void* stream);

/* ---- brush scores: the reference's colour and transparency metrics (csrc/nb_metrics.hip) -----------------------------------------
 * Evaluation masks of K drawings, once per set of drawings.  geom [k,r,r] fp32, 0 = stroke.  blur [k,r,r] =
 * default_gaussian_smoothing applied twice (forger/metrics/geom_metric.py:126-129, 153): a 5x5 Gaussian, sigma 1, normalised to sum 1,
 * zero padding 2 at EACH application, so what the first application would put outside the image is zero for the second.  mask
 * [k,r,r] bytes: bit 0 = background, blur > 0.999f; bit 1 = foreground, geom < 0.3f (geom_metric.py:156-159).  n_bg[k] / n_fg[k] =
 * the set bits of each drawing's mask (cleared and counted on `stream`, integer arithmetic).  One launch, 25 taps per pass in fp32:
 * within 4e-6 of float64 on values in 0..1.  Values outside 0..1, infinities and NaN do not fault; what they give is unspecified.
 * k == 0: NB_OK without a launch.  NB_EINVAL: a null pointer, k outside 0..65535, r outside 1..8192, a float / int pointer not 4-byte
 * aligned. */
int nb_eval_masks_f32(const float* geom, int k, int r, float* blur, uint8_t* mask, int32_t* n_bg, int32_t* n_fg, void* stream);

/* Workgroups that share one image in nb_brush_metrics_f32: `partials` holds n * NB_BRUSH_METRICS_PARTS * 4 floats. */
#define NB_BRUSH_METRICS_PARTS 16

/* The per-image sums behind LAB_E%, LAB_L2 (compute_lab_metrics, forger/metrics/color_metric.py:29-70, with rgb2lab of
 * forger/util/color.py:52-140) and BG_CLARITY_MEAN (compute_transparency_metrics, geom_metric.py:152-158) of n renders, in one pass.
 * Render i is four dense planes r, g, b, alpha of r * r floats at renders + i * stride_n (stride_n >= 4 * r * r; a view into a larger
 * tensor is read in place), in 0..1; its target colour is target_rgb[3 i .. 3 i + 2]; it uses drawing i % k of geom [k,r,r] and of
 * mask [k,r,r] (nb_eval_masks_f32; only bit 0 is read).  Per pixel: rgb = alpha * rgb + (1 - alpha) unless ignore_transparency,
 * sRGB -> linear (split at 0.04045, exponent 2.4), XYZ, f() with its linear branch below (6/29)^3 and 1e-8 added inside the cube
 * root, Lab, dE = |Lab - Lab(target)|_2 (the target's Lab computed once per workgroup).  With the float weight w = 1 - geom:
 *   sums[4 i + 0] = sum w dE      sums[4 i + 1] = sum w [dE > lab_thresh]      sums[4 i + 2] = sum w      sums[4 i + 3] = sum of alpha
 *                                                                                                          over background pixels
 * alpha [n, r*r] receives every render's alpha plane, dense, so that nb_masked_kth_largest_f32 can pool the images of a brush;
 * deltas [n, r*r] (may be null) receives dE.  NB_BRUSH_METRICS_PARTS workgroups share an image and leave partial sums in `partials`;
 * a second small launch of the same call adds them in a fixed order: no float atomics, the same input gives the same bits.  Planes
 * are read in 16-byte vectors when r * r and stride_n are multiples of four and renders, geom, alpha and deltas are 16-byte aligned,
 * otherwise pixel by pixel (any float may start a plane).  Only enqueues on `stream`: no allocation, no host wait, capturable.
 * Values outside 0..1, infinities and NaN do not fault; what they give is unspecified.  n == 0: NB_OK without a launch.
 * NB_EINVAL: a null pointer (deltas excepted), k < 1, r outside 1..8192, n outside 0..2^24, stride_n < 4 r r, a float pointer not
 * 4-byte aligned. */
int nb_brush_metrics_f32(const float* renders, long long stride_n, const float* target_rgb, const float* geom, const uint8_t* mask,
                         int k, int r, int n, float lab_thresh, int ignore_transparency, float* sums, float* alpha, float* deltas,
                         float* partials, void* stream);

/* ---- inputs of the perceptual brush scores (csrc/nb_metric_patches.hip): what compute_uniform_bg_lpips_metric
 * (forger/metrics/geom_metric.py:207-262) and compute_lpips_across_geo (geom_metric.py:190-204) do to a batch of renders before the
 * LPIPS network sees it.  Renders are read in place as nb_brush_metrics_f32 reads them: four dense planes r, g, b, alpha of r * r
 * floats at renders + i * stride_n (stride_n >= 4 r r), in 0..1; image i lies on drawing i % k.  fp32 throughout, no float atomics:
 * the same input gives the same bits.  The entries only enqueue on `stream`: no allocation, no host wait.  Values outside 0..1,
 * infinities and NaN do not fault; what they give is unspecified.
 *
 * The guidance of the background metrics, once per set of drawings.  geom [k,r,r] fp32, 0 = stroke.  blur1 [k,r,r] =
 * default_gaussian_smoothing applied ONCE (geom_metric.py:126-129, 235): the 5x5 Gaussian, sigma 1, normalised to sum 1, zero padding
 * 2, with the weights of nb_eval_masks_f32; within 2e-6 of float64 on values in 0..1.  n_bg[k] = the pixels with blur1 > 0.99f
 * (BG_THRESH of geom_metric.py:238-239; NOT the 0.999 on the twice-blurred guidance of nb_eval_masks_f32), cleared and counted on
 * `stream` in integer arithmetic.  k == 0: NB_OK without a launch.  NB_EINVAL: a null pointer, k outside 0..65535, r outside
 * 1..8192, a pointer not 4-byte aligned. */
int nb_bg_guidance_f32(const float* geom, int k, int r, float* blur1, int32_t* n_bg, void* stream);

/* Workgroups that share one image in nb_bg_mean_colors_f32: `partials` holds n * NB_BG_MEAN_PARTS * 3 floats. */
#define NB_BG_MEAN_PARTS 16

/* The mean background colour of n renders (geom_metric.py:232-241): mean[3 i + c] = sum over the pixels with blur1 > 0.99f of
 * (alpha * rgb_c + (1 - alpha)), divided by max(n_bg[i % k], 1) -- an image without background gets zeros.  blur1 [k,r,r] and n_bg [k]
 * are nb_bg_guidance_f32's.  NB_BG_MEAN_PARTS workgroups share an image and leave partial sums in `partials`; a second small launch
 * of the same call adds them in a fixed order and divides.  16-byte vectors when r * r and stride_n are multiples of four and renders
 * and blur1 are 16-byte aligned, otherwise pixel by pixel.  n == 0: NB_OK without a launch.  NB_EINVAL: a null pointer, k < 1, r
 * outside 1..8192, n outside 0..2^24, stride_n < 4 r r, a pointer not 4-byte aligned. */
int nb_bg_mean_colors_f32(const float* renders, long long stride_n, const float* blur1, const int32_t* n_bg, int k, int r, int n,
                          float* partials, float* mean, void* stream);

#define NB_METRIC_PAIRS_TRANSPOSE 1   /* the second patch with rows and columns exchanged (permute(0,1,3,2), geom_metric.py:250) */
#define NB_METRIC_PAIRS_MASKED 2      /* fill what is not background in BOTH patches with the first image's mean colour (:255-257) */

/* The LPIPS input of n pairs of patches, both sides in ONE buffer: out [2n,3,p,p], out[i] the first and out[n + i] the second patch
 * of pair i, so that the trunk runs once over 2n images.  The first patch is the p x p window of image i at (row, column) =
 * off0[2 i], off0[2 i + 1]; the second the window of image j = src1[i] (src1 NULL: j = i) at off1[2 i], off1[2 i + 1], transposed
 * with NB_METRIC_PAIRS_TRANSPOSE.  Every pixel is composited over white, alpha * rgb + (1 - alpha).  With NB_METRIC_PAIRS_MASKED a
 * pixel is background where blur1 of BOTH patches exceeds 0.99f (image j on drawing j % k, its patch transposed first); background
 * pixels keep their colour, every other pixel of both patches takes mean[3 i .. 3 i + 2] -- the FIRST image's, also for a permuted
 * second patch (geom_metric.py:256-257).  Both patches are then scaled by * 2 - 1 (:258-259).  Without MASKED (blur1 and mean may be
 * NULL) and without TRANSPOSE, with p = r and zero offsets: the pairs of compute_lpips_across_geo for the permutation src1.
 * An offset is clamped into 0..r - p and src1[i] into 0..n - 1 on the device (they cannot be checked on the host).  One launch; the
 * transposed patch is staged through a padded LDS tile, so both patches are read along image rows.  16-byte stores (and loads, for
 * windows whose column offset is a multiple of four) when p, r and stride_n are multiples of four and renders, blur1 and out are
 * 16-byte aligned; otherwise element by element, any alignment of the output planes (p odd).  n == 0: NB_OK without a launch.
 * NB_EINVAL: a null pointer (src1 excepted; blur1 and mean without MASKED), unknown flags, k < 1, r outside 1..8192, p outside 1..r,
 * n outside 0..2^24, n * ceil(p / 32)^2 above 2^31 - 1, stride_n < 4 r r, a pointer not 4-byte aligned. */
int nb_metric_pairs_f32(const float* renders, long long stride_n, const float* blur1, const float* mean, const int32_t* off0,
                        const int32_t* off1, const int32_t* src1, int k, int r, int p, int n, int flags, float* out, void* stream);

/* ---- inputs of the stitching scores (csrc/nb_stitch_metrics.hip): what the reference's metric loop (forger/metrics/metric_main.py:
 * 181-200) and compute_stitching_metrics (forger/metrics/geom_metric.py:165-187) do around the two generator passes of
 * RandomStitcher.generate_with_stitching (forger/train/stitching.py:212-267).  fp32 throughout, no float atomics: the same input
 * gives the same bits.  The entries only enqueue on `stream`: no allocation, no host wait.
 *
 * The generator's geometry input of n windows of full-size drawings: out [n,1,r,r] fp32, out[i] = the r x r window of drawing
 * draw[i] of drawings [k,d,d] uint8 (0 = stroke) at (row, column) = off[2 i], off[2 i + 1], value / 255 in correctly rounded fp32.
 * draw and off live on the device: an index is clamped into 0..k - 1 and an offset into 0..d - r there.  16-byte stores when r is a
 * multiple of four and out is 16-byte aligned.  n == 0: NB_OK without a launch.  NB_EINVAL: a null pointer, k outside 1..65535, r
 * outside 1..8192, d outside r..32768, n outside 0..2^24, draw, off or out not 4-byte aligned. */
int nb_stitch_crops_u8(const uint8_t* drawings, int k, int d, const int32_t* draw, const int32_t* off, int n, int r, float* out,
                       void* stream);

/* Workgroups that share one sample in nb_stitch_pairs_f32: `partials` holds n * NB_STITCH_PARTS * 2 floats. */
#define NB_STITCH_PARTS 32

/* The LPIPS input and the L1 sums of the 2n pairs of n stitched samples.  fake: 2n raw generator images of three dense planes of
 * r * r floats at fake + j * stride_n (stride_n >= 3 r r: a view is read in place); images 0..n-1 are the first crops (fake1),
 * n..2n-1 the second (fake2).  rects_a / rects_b [n,8] int32 on the device, per sample (area1, area2), each (rstart, cstart, rend,
 * cend) with exclusive ends: rects_a those of compute_overlaps(crop1, offset_crop(crop2)) (stitching.py:248), rects_b those of
 * compute_overlaps(offset_crop(crop1), crop2) (:252).  With crop(img) = img[:, margin:r - 2 margin, margin:r - 2 margin] -- the
 * reference's ASYMMETRIC crop (geom_metric.py:173-177), s = r - 3 margin wide -- out [4n,3,s,s] is, in the row convention of
 * nb_metric_pairs_f32 (first sides, then second sides):
 *     out[i]      = crop(fake1[i])                         out[2n + i] = crop(fake1[i] with fake2[i]'s area2 of rects_a in area1)
 *     out[n + i]  = crop(fake2[i])                         out[3n + i] = crop(fake2[i] with fake1[i]'s area1 of rects_b in area2)
 * (CropHelper.composite, stitching.py:161-179, 249, 253), every value a copy of an input float (nothing is rescaled), and
 * l1[j] = sum over the 3 s s entries of |out[j] - out[2n + j]| for j < 2n: only a rectangle's part inside the crop window adds to
 * it.  A rectangle pair that is empty (zero or negative extent), leaves 0..r or whose two extents differ means "no composite": the
 * second side equals the first and the sum is 0.  NB_STITCH_PARTS workgroups share a sample and leave partial sums in `partials`; a
 * second small launch of the same call adds them in a fixed order.  16-byte loads and stores when s, r, margin and stride_n are
 * multiples of four and fake and out are 16-byte aligned; otherwise element by element.  n == 0: NB_OK without a launch.
 * NB_EINVAL: a null pointer, r outside 1..8192, n outside 0..2^22, margin < 0 or 3 margin >= r, stride_n < 3 r r, a pointer not
 * 4-byte aligned. */
int nb_stitch_pairs_f32(const float* fake, long long stride_n, const int32_t* rects_a, const int32_t* rects_b, int n, int r, int margin,
                        float* out, float* l1, float* partials, void* stream);

/* ---- clarity optimisation of brushes (csrc/nb_clarity.hip): what one step of run_one_clarity_opt (scripts/opt_clarity_main.py:93-167)
 * does around the generator, for k brushes at once.  The state of k brushes is an arena [k, p] of floats (row stride given per call):
 * a row is W+ (nw floats) followed by noise planes.  NbClarityPlanes lists the planes in the order of their offsets: side (a power of
 * two in 4..256) and offset in floats from the start of a row.  It is a HOST struct: every entry checks it against nw and p before any
 * HIP call (NB_EINVAL: more than NB_CLARITY_MAX_PLANES, a side that is unsupported, planes that overlap, precede nw or leave the row)
 * and hands it to its kernels by value, so no launch can index outside a row.  fp32 throughout; no float atomics: partial sums are
 * left in caller-supplied scratch and added in a fixed order, so the same input gives the same bits, and row i of a k-row call equals
 * the one-row call on that row.  The entries only enqueue on `stream`: no allocation, no host wait.  k == 0: NB_OK without a launch. */
#define NB_CLARITY_MAX_PLANES 32
#define NB_CLARITY_LOSS_PARTS 8       /* workgroups that share one sample in nb_clarity_loss_f32 */
#define NB_CLARITY_CHUNK 1024         /* floats of a row one workgroup of nb_clarity_step_f32 updates */
typedef struct NbClarityPlanes {
    int32_t n;
    int32_t res[NB_CLARITY_MAX_PLANES];
    int32_t off[NB_CLARITY_MAX_PLANES];
} NbClarityPlanes;

/* Floats of scratch that nb_noise_reg_f32 and nb_clarity_step_f32 need for k rows of this layout (the larger of the two); -1 with
 * nb_last_error set if the layout is invalid or k is outside 0..65535. */
long long nb_clarity_scratch_floats(const NbClarityPlanes* planes, int nw, long long p, int k);

/* The loss 'w_iou_inv*iou_inv(uvs)+w_iou*iou(u)+w_l1*l1(fake_orig)' (forger/train/losses.py:453-474, 501-530; compute_iou in its
 * per-sample form, :649-666, eps 1e-8; l1_loss with mean reduction) of k brushes on b drawings each.  Sample n = brush * b + drawing:
 * uvs / img / target are three dense planes of r * r floats at <base> + n * <stride_n> (stride_n >= 3 r r: views are read in place);
 * geom [b,r,r] is the truth, 1 = background, shared by the brushes.  With s = uvs[2], u = uvs[0], g = geom, t = 1 - g, per sample
 *   I_s = sum s g,  U_s = sum (s + g) - I_s + eps,  I_u = sum u t,  U_u = sum (u + t) - I_u + eps,  L = sum |img - target|
 * sums [k*b, 8] receives {I_s, U_s, I_u, U_u, L, 0, 0, 0} (what the backward entry reads), out [k, 4] per brush
 *   {1 - mean_b I_s / U_s,  1 - mean_b I_u / U_u,  sum_b L / (3 b r r),  the weighted sum of the three}.
 * partials: k * b * NB_CLARITY_LOSS_PARTS * 8 floats.  Two launches.  NB_EINVAL: a null pointer, k < 0, b < 1, r outside 1..4096,
 * k * b > 65535, a stride below 3 r r, a pointer not 4-byte aligned. */
int nb_clarity_loss_f32(const float* uvs, long long uvs_stride_n, const float* img, long long img_stride_n, const float* target,
                        long long target_stride_n, const float* geom, int k, int b, int r, float w_iou_inv, float w_iou, float w_l1,
                        float* out, float* sums, float* partials, void* stream);

/* Gradient of out[brush, 3] (times gscale[brush]; gscale NULL = 1) from the sums of nb_clarity_loss_f32, dense outputs
 * d_uvs [k*b,3,r,r] and d_img [k*b,3,r,r]:
 *   d_uvs[2] = -w_iou_inv / b * (g U_s - I_s (1 - g)) / U_s^2      d_uvs[0] = -w_iou / b * (t U_u - I_u (1 - t)) / U_u^2      d_uvs[1] = 0
 *   d_img = w_l1 * sign(img - target) / (3 b r r), sign(0) = 0.
 * One launch.  NB_EINVAL as for the forward entry. */
int nb_clarity_loss_bwd_f32(const float* img, long long img_stride_n, const float* target, long long target_stride_n, const float* geom,
                            const float* sums, const float* gscale, int k, int b, int r, float w_iou_inv, float w_iou, float w_l1,
                            float* d_uvs, float* d_img, void* stream);

/* The noise regulariser of opt_clarity_main.py:127-137 over all planes of k rows, value and gradient.  Per plane and level l (sides
 * res, res / 2, ... down to 8; one level for res <= 8): n_l = the 2x2 mean of n_(l-1), a_l = mean(n_l * roll_x n_l), b_l likewise in
 * y, and the value is the sum of a_l^2 + b_l^2.  reg [k] receives the value of each row (summed over planes in their order).  The
 * gradient at a level-0 pixel, sum_l 4^-l [2 a_l / N_l (left + right) + 2 b_l / N_l (up + down)] of n_l around (y >> l, x >> l) with
 * wrap-around, is ADDED times `weight` (regularize_noise_weight) to grad [k, p] (grad NULL: the value only).  Two launches: the sums
 * per tile with the pyramid written to scratch, then the gradient.  scratch: nb_clarity_scratch_floats.  NB_EINVAL: a null pointer
 * (grad excepted), an invalid layout, k outside 0..65535, a row stride below p, a pointer not 4-byte aligned, scratch too small. */
int nb_noise_reg_f32(const float* arena, long long row_stride, long long p, int nw, const NbClarityPlanes* planes, int k, float weight,
                     float* grad, long long grad_stride, float* reg, float* scratch, long long scratch_floats, void* stream);

/* One optimiser step on the arena: Adam with torch.optim.Adam's defaults and arithmetic (betas 0.9 / 0.999, eps 1e-8, bias-corrected;
 * opt_clarity_main.py:86, 159-161) over all k * p floats -- arena, grad, m, v share the layout and row_stride; lr and the step count
 * t >= 1 are host scalars -- then, per noise plane, n -= mean(n); n *= rsqrt(mean(n^2)) (opt_clarity_main.py:163-167).  W+ is not
 * normalised.  Two launches: the update with each chunk's sums of n and n^2, then the normalisation.  scratch:
 * nb_clarity_scratch_floats.  NB_EINVAL: a null pointer, an invalid layout, k outside 0..65535, t < 1, row_stride < p, a pointer not
 * 4-byte aligned, scratch too small. */
int nb_clarity_step_f32(float* arena, const float* grad, float* m, float* v, long long row_stride, long long p, int nw,
                        const NbClarityPlanes* planes, int k, float lr, int t, float* scratch, long long scratch_floats, void* stream);

/* ---- brush projection (csrc/nb_projection.hip): the loss that project() (scripts/project_main.py:38-224) computes around the
 * generator, for k exemplars of b patches each.  Sample n = exemplar * b + patch; every exemplar has its own drawings.  Tensors of
 * samples are three dense planes of r * r floats at <base> + n * <stride_n> (stride_n >= 3 r r: views are read in place).  Planes are
 * read in 16-byte vectors when r * r and every stride are multiples of four and every plane pointer is 16-byte aligned (mask: 4-byte),
 * otherwise pixel by pixel (any float may start a plane).  fp32 throughout; no float atomics: NB_PROJECTION_PARTS workgroups share a
 * sample and leave partial sums in caller-supplied `partials`, a small second launch adds them in a fixed order, so the same input
 * gives the same bits, and row i of a k-row call equals the one-row call on that row.  The entries only enqueue on `stream`: no
 * allocation, no host wait.  k == 0: NB_OK without a launch.  NB_EINVAL for all three: a null pointer (the optional ones excepted),
 * k < 0, b < 1, r outside 1..4096, k * b > 65535, a stride below 3 r r, a float / int pointer not 4-byte aligned. */
#define NB_PROJECTION_PARTS 8         /* workgroups that share one sample */

/* Once per pass.  blur [k*b,r,r] dense: the drawings (0 = stroke) under the 5x5 sigma-1 Gaussian applied twice with zero padding
 * (what nb_eval_masks_f32 writes); target: the exemplar patches.  mask [k*b,r,r] bytes: bit 0 = background, blur >= 0.999f; bit 1 =
 * foreground, blur < 0.1f (get_conservative_fg_bg, forger/metrics/geom_metric.py:132-140; note >= and 0.1, which differ from
 * nb_eval_masks_f32's).  counts [k,2] int32 = {n_fg, n_bg} over an exemplar's b patches; bg_color [k,3] = per channel the mean of
 * target over the exemplar's background pixels (compute_masked_color, project_main.py:248-250), zeros where n_bg == 0.
 * partials: k * b * NB_PROJECTION_PARTS * 8 floats.  Two launches. */
int nb_projection_masks_f32(const float* blur, const float* target, long long target_stride_n, int k, int b, int r, uint8_t* mask,
                            int32_t* counts, float* bg_color, float* partials, void* stream);

/* The forward.  colors [k*b,3,3] dense, indexed [c][j] as in compose_stroke (forger/viz/visualize.py:315-323).  With composite != 0
 * (composite_with_bg_color / composite_with_bg_image, project_main.py:227-245):
 *   stroke[c] = sum_j uvs[j] colors[c][j],   synth[c] = stroke[c] (1 - uvs[2]) + bg[c] uvs[2],
 * bg = bg_image (samples of stride bg_stride_n) if it is not NULL, else the exemplar's bg_color [k,3]; synth [k*b,3,r,r] is written,
 * dense; img is not read and may be NULL.  With composite == 0: synth = img, nothing is written; colors, bg_image, bg_color and synth
 * are not read and may be NULL.  out [k,3] per exemplar (project_main.py:164-168, with mask and counts of nb_projection_masks_f32):
 *   l1 = sum over foreground pixels and 3 channels of |target - synth| / (3 n_fg),   bg = sum over background pixels of
 *   (1 - uvs[2]) / n_bg,   w_l1 l1 + w_bg bg;   an item whose count is zero is 0.
 * partials: k * b * NB_PROJECTION_PARTS * 4 floats.  Two launches. */
int nb_projection_loss_f32(const float* uvs, long long uvs_stride_n, const float* colors, const float* img, long long img_stride_n,
                           const float* target, long long target_stride_n, const float* bg_image, long long bg_stride_n,
                           const float* bg_color, const uint8_t* mask, const int32_t* counts, int k, int b, int r, int composite,
                           float w_l1, float w_bg, float* synth, float* out, float* partials, void* stream);

/* The backward: the forward's inputs, an optional upstream gradient d_synth [k*b,3,r,r] (dense; NULL = none) of synth and an optional
 * gscale [k] (NULL = 1) that multiplies the gradient of out[exemplar, 2].  With
 *   G[c] = d_synth[c] + gscale w_l1 [fg] sign(synth[c] - target[c]) / (3 n_fg),   sign(0) = 0,   a = 1 - uvs[2]:
 * composite:     d_uvs[j] = sum_c G[c] colors[c][j] a  for j = 0, 1
 *                d_uvs[2] = sum_c G[c] (colors[c][2] a - stroke[c] + bg[c]) - gscale w_bg [bg] / n_bg
 *                d_colors [k*b,3,3]: d_colors[n][c][j] = sum over pixels of G[c] uvs[j] a   (through partials, in a fixed order)
 * no composite:  d_img = G,   d_uvs[2] = -gscale w_bg [bg] / n_bg,   d_uvs[0] = d_uvs[1] = 0.
 * A count of zero gives its item the gradient 0.  d_uvs [k*b,3,r,r] dense is always written; d_img [k*b,3,r,r] dense only without
 * composite (else it may be NULL); d_colors and partials (k * b * NB_PROJECTION_PARTS * 16 floats) only with composite.  One launch,
 * plus the finishing launch for d_colors. */
int nb_projection_loss_bwd_f32(const float* uvs, long long uvs_stride_n, const float* colors, const float* img, long long img_stride_n,
                               const float* target, long long target_stride_n, const float* bg_image, long long bg_stride_n,
                               const float* bg_color, const uint8_t* mask, const int32_t* counts, const float* d_synth, const float* gscale,
                               int k, int b, int r, int composite, float w_l1, float w_bg, float* d_uvs, float* d_img, float* d_colors,
                               float* partials, void* stream);

/* ---- LPIPS network (csrc/nb_lpips.hip; perceptual.LPIPS): what surrounds the trunk's convolutions.  All tensors fp32, NCHW, dense.
 * No float atomics: the same input gives the same bits, and sample i of an n-sample call equals the one-sample call on it.  The entries
 * only enqueue on `stream`: no allocation, no host wait.  n == 0: NB_OK without a launch.  NB_EINVAL for all: a null pointer (the
 * optional ones excepted), n outside 0..65535 (nb_lpips_scale_f32: n < 0), a size below 1, c * h * w of 2^31 or more, a pointer not
 * 4-byte aligned. */
#define NB_LPIPS_SPLIT_MAX_HW 1024    /* nb_lpips_head_f32 splits the channels over a workgroup for maps of h * w <= this ... */
#define NB_LPIPS_SPLIT_MIN_C  64      /* ... with at least this many channels; one thread per pixel otherwise */

/* The scaling layer: y[n,c,:] = (x[n,c,:] - shift[c]) / scale[c] over hw pixels per plane; shift NULL = 0, which is the layer's
 * backward (dx = dy / scale). */
int nb_lpips_scale_f32(const float* x, const float* shift, const float* scale, float* y, int n, int c, long long hw, void* stream);

/* Bias + ReLU + tap + max-pool behind a convolution, one launch: tap [n,c,h,w] = max(x + bias[c], 0) and, with window 2 or 3,
 * pooled [n,c,ph,pw] = the maximum of tap over windows of that side, stride 2, no padding, floor mode (ph = (h - window) / 2 + 1).
 * window 0: no pool, pooled is not written and may be NULL.  One add and maxima, each exactly rounded.  NB_EINVAL also for another
 * window, or one above h or w. */
int nb_lpips_relu_pool_f32(const float* x, const float* bias, float* tap, float* pooled, int n, int c, int h, int w, int window, void* stream);

/* Its backward, one launch: d_x [n,c,h,w] from tap (the forward's) and the gradients d_tap [n,c,h,w] and d_pooled [n,c,ph,pw], either of
 * which may be NULL.  A window's gradient goes to its FIRST maximum in row-major order; a pixel takes d_tap, then its windows in their
 * order.  d_x = 0 where tap == 0.  NB_EINVAL also for d_pooled with window 0. */
int nb_lpips_relu_pool_bwd_f32(const float* tap, const float* d_tap, const float* d_pooled, float* d_x, int n, int c, int h, int w, int window,
                               void* stream);

/* Workgroups that share one sample in nb_lpips_head_f32 for maps of c channels and hw pixels (the floats of `partials` per sample); -1
 * with nb_last_error set for sizes below 1. */
long long nb_lpips_head_parts(int c, int hw);

/* One level of the head.  f0, f1 [n,c,hw] raw feature maps, w [c] (any sign).  Per pixel, in one pass over the channels, the sums
 *   A = sum f0^2,  B = sum f1^2,  P = sum w f0^2,  Q = sum w f1^2,  X = sum w f0 f1      (carried in fp64),
 * then with i0 = 1 / (sqrt(A) + 1e-10), i1 = 1 / (sqrt(B) + 1e-10), each 0 where its sum is 0:
 *   d = P i0^2 + Q i1^2 - 2 X i0 i1  =  sum_c w_c (f0_c i0 - f1_c i1)^2.
 * kept [3, n, hw] receives i0, sqrt(B) and Q i1 - X i0 = sum_c w_c e_c f1_c (e = u1 - u0), which the backward reads.  partials
 * [n * nb_lpips_head_parts(c, hw)] receives the workgroups' sums of d; the finishing launch adds them in their order and ADDS
 * sum / hw into acc [n] (the caller zeroes acc before the first level).  Two launches. */
int nb_lpips_head_f32(const float* f0, const float* f1, const float* w, int n, int c, int hw, float* kept, float* partials, float* acc,
                      void* stream);

/* Gradient of sum_n g[n] * mean_pixels d with respect to f1 (f0 takes none): with s = kept[1], n1 = s + 1e-10, e_k = f1_k / n1 - f0_k i0,
 *   d_f1_k = g[n] / hw * (2 w_k e_k / n1 - f1_k * 2 kept[2] / (n1^2 s)),   0 where s == 0
 * (the package's sqrt gives NaN there).  accumulate != 0: added to what d_f1 [n,c,hw] holds.  One launch. */
int nb_lpips_head_bwd_f32(const float* f0, const float* f1, const float* w, const float* kept, const float* g, int n, int c, int hw, int accumulate,
                          float* d_f1, void* stream);

/* ---- geometry encoder (forger/experimental/autoenc/simple_autoencoder.py:88-121, 155-199,
 * 251-261).  Every layer is conv(reflect padding) + bias + LeakyReLU(slope) with eval-mode BatchNorm folded into
 * the weights and bias by the caller.  Activations between layers travel in the H2 format of the split-f16 convs. */

/* Stem: 1 -> 64 channels, 7x7, reflect padding 3.  x fp32 [n,1,h,w] (h % 16 == 0, w % 32 == 0), w50 [64][50] =
 * folded weights [c_out][ky*7+kx] padded with one zero, y_h2 = H2 [n,8,2,h,w,8].  preproc (autoenc/base.py:30-52):
 * 0 none, 1 '-11inverse' (1-x)*2-1, 2 'inverse' 1-x.  Split-f16 products (three v_mfma_f32_32x32x16_f16 per K step over the
 * hi / lo f16 halves of image and weights: fp32-grade, within 2e-6 of the largest pre-bias output of float64). */
int nb_enc_stem7x7_f32_h2(const float* x, const float* w50, const float* bias, void* y_h2, int n, int h, int w,
                          int preproc, float slope, void* stream);

/* 3x3 conv, stride 1 or 2, reflect padding 1, split-f16 products.  x_h2: H2 [n, c_in, h_in, w_in]; w_h3: hi/lo f16
 * [ceil(c_in/16)][3][3][2][2][ceil128(c_out)][8]; exactly one of y_f32 (fp32 NCHW [n,c_out,h_in/stride,w_in/stride])
 * and y_h2 (H2, c_out % 8 == 0) is non-NULL.  Output sizes: a multiple of 32 wide with rows % 8 == 0 (8 x 32 tiles), any other
 * multiple of 16 wide with rows % 16 == 0 (16 x 16 tiles: 16, 48, 80 ...), or -- with c_in % 16 == 0 -- a power of two >= 4 wide with
 * any number of rows (the 32-position split-K tiles: rows that do not fill the last tile are masked).  Where both forms fit and c_in >= 32,
 * under-filled launches (<= 48 large-tile workgroups) and layers with c_out <= 32 take the split-K tiles. */
int nb_enc_conv3x3_h3(const void* x_h2, int c_in, const void* w_h3, const float* bias, float* y_f32, void* y_h2, int n,
                      int h_in, int w_in, int c_out, int stride, float slope, void* stream);

/* The same convolution writing straight into a CONSUMER's split-f16 operand tensor (the generator layer that takes these
 * geometry features as extra input channels, networks_modified.py:218-219 `torch.cat`): the result times
 * oscale[n * oscale_stride + co] (the consumer's styles of those channels; NULL = 1) goes into channel groups
 * cg0 .. cg0 + c_out/8 - 1 of y_h2 [n][c8_total][2][h][w][8]; out_fmt 0 = H2 (hi/lo f16), 1 = "f8" (hi f16 + fp8
 * correction operands: c_out % 16 == 0, cg0 even).  Removes the fp32 round trip + nb_pack_h2*_part_f32 pass.  Needs an output size
 * the 8 x 32 or 16 x 16 tiles take (the split-K tiles have no hand-off), c8_total >= cg0 + c_out/8 and oscale_stride >= c_out;
 * anything else is NB_EINVAL with nothing written.  Words of y_h2 outside those channel groups are not touched. */
int nb_enc_conv3x3_h3_handoff(const void* x_h2, int c_in, const void* w_h3, const float* bias, void* y_h2,
                              const float* oscale, int oscale_stride, int c8_total, int cg0, int out_fmt,
                              int n, int h_in, int w_in, int c_out, int stride, float slope, void* stream);

/* Bilinear x2, align_corners=True (nn.Upsample in ScaleUp, simple_autoencoder.py:106-121): fp32 NCHW [n,c,h,w]
 * (c % 8 == 0) -> H2 [n, c, 2h, 2w]. */
int nb_enc_upsample2x_h2(const float* x, void* y_h2, int n, int c, int h, int w, void* stream);

/* The encoder layers with the "f8" operand format BETWEEN them (the format of the generator's f8 arithmetic mode: hi f16
 * + fp8 correction operands per 16-channel chunk; one f16 + half an fp8 MFMA per tap instead of three f16 MFMAs).
 * in_fmt / out_fmt: 0 = H2, 1 = f8 (c % 16 == 0).  For in_fmt 1 the weights are packed like the generator's f8 weights:
 * lo slot of chunk group 0 = fp8(w), of group 1 = fp8((w - f16(w)) 2^11), over the 16 channels of the chunk
 * ([ceil(c_in/16)][3][3][2][2][ceil128(c_out)][8] containers as for H2).  nb_enc_conv3x3_ex is the general form of the
 * two entry points above (oscale / c8_total / cg0 as in the hand-off; c8_total 0 = a plain tensor of c_out channels). */
int nb_enc_stem7x7_f32_h2_ex(const float* x, const float* w50, const float* bias, void* y_h2, int out_fmt, int n, int h, int w,
                             int preproc, float slope, void* stream);
int nb_enc_conv3x3_ex(const void* x, int c_in, const void* wts, const float* bias, float* y_f32, void* y_h2,
                      const float* oscale, int oscale_stride, int c8_total, int cg0, int in_fmt, int out_fmt,
                      int n, int h_in, int w_in, int c_out, int stride, float slope, void* stream);

/* Stem + first stride-2 stage in ONE launch (simple_autoencoder.py:155-176: _SingleConvolution 1 -> 64, 7 x 7, followed by the first
 * _Downsample stage 64 -> c_out, stride 2): the result of nb_enc_stem7x7_f32_h2_ex(out_fmt 1) followed by nb_enc_conv3x3_ex(in_fmt 1,
 * stride 2) without the 64-channel full-resolution tensor between them -- each workgroup computes the stem outputs its tile needs on the
 * matrix pipe, chunk by chunk, straight into LDS in operand format.  x fp32 [n,1,h,w] (h % 16 == 0, w % 64 == 0); w50 / bias0 / preproc
 * as nb_enc_stem7x7_f32_h2; wts1: the stage's weights in "f8" format (c_in = 64), bias1 [c_out], c_out % 16 == 0; y_h2
 * [n, c_out, h/2, w/2] in format out_fmt (0 = H2, 1 = f8).  Same split-f16 products; per stem output the summation order differs
 * from the stem kernel's (results agree to fp32 rounding, not bit for bit). */
int nb_enc_stem_conv3x3_f8(const float* x, const float* w50, const float* bias0, int preproc, const void* wts1, const float* bias1,
                           void* y_h2, int out_fmt, int n, int h, int w, int c_out, float slope, void* stream);

/* Stride-2 3x3 correlation WITHOUT padding on the same kernel -- the strided half of conv2d_resample's down-sampling branch
 * (conv2d_resample.py:96-113) and the input gradient of its up-sampling branch (:124-147), which cuDNN runs for the reference:
 * x H2 [n][c8][2][2ho+1][2wo+1][8], weights as above, y fp32 [n][c_out][ho][wo] = oscale[n][co] * (bias[co] + sum_{ci,a,b}
 * x[n,ci,2i+a,2j+b] w[co,ci,a,b]); oscale may be NULL.  Output sizes: wo % 32 == 0 and ho % 8 == 0, or wo % 16 == 0 and ho % 16 == 0
 * (the large tiles only: the split-K tiles of nb_enc_conv3x3_h3 have no unpadded form). */
int nb_conv3x3_s2_valid_h3(const void* x_h2, int c_in, const void* w_h3, const float* bias, const float* oscale, int oscale_stride,
                           float* y_f32, int n, int h_in, int w_in, int c_out, void* stream);
int nb_enc_upsample2x_h2_ex(const float* x, void* y_h2, int out_fmt, int n, int c, int h, int w, void* stream);

/* Host-side helper (no GPU): repack W[c_out,c_in,3,3] into the zero-padded
 * wpk[ceil8(c_in)][9][ceil32(c_out)] and wsq[c_in][c_out] = sum_k W^2.  Either output may be NULL. */
int nb_pack_conv_weight(const float* w, int c_out, int c_in, float* wpk, float* wsq);

/* ---- device weight packers (csrc/nb_weight_pack.hip): the packed forms the generator layers take, built from the fp32 weight
 * W[c_out,c_in,3,3] on the DEVICE (w and every output are device pointers; enqueue only).  Bit for bit what the package's torch
 * packers (ops.py) produce. */

/* wpk [ceil8(c_in)][9][ceil32(c_out)] zero padded (nb_modconv3x3_f32) and wsq [c_in][c_out] = sum_k W[o,i,k]^2, summed in the
 * order torch's reduction kernel uses on this platform for 9 contiguous elements: ((s0 + s8 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)).
 * Either output may be NULL. */
int nb_pack_conv_weight_dev(const float* w, int c_out, int c_in, float* wpk, float* wsq, void* stream);
/* The "f8" weight format (nb_pack_conv_weight_h3's container, lo slots in fp8 e4m3; see the f8 section above). */
int nb_pack_conv_weight_h3f8_dev(const float* w, int c_out, int c_in, void* out, void* stream);
/* The four up=2 phase kernels of nb_modconv3x3_up2_small_h3 (W folded with the 4x4 resample filter f [4,4], the fold summed in
 * float64 and rounded to fp32), each in the nb_pack_conv_weight_h3 format, back to back. */
int nb_pack_conv_weight_h3_up2_dev(const float* w, const float* resample_filter, int c_out, int c_in, void* out, void* stream);

/* ---- the whole generator behind one handle (csrc/nb_generator.hip; tables and planner: nb_gen_plan.hip, encoder: nb_gen_encoder.hip) ----
 * For C / C++ hosts: create a generator from its fp32 weights once, then enqueue whole forward passes (mapping, styles, noise,
 * every synthesis layer, the fused ToRGB + compositing) with one call.  The per-batch kernel choices are those of the package's
 * Python pass (SynthesisNetwork) at the same batch size, and so are the results, bit for bit.
 *
 * Exceptions to the header's rules: nb_generator_create allocates device memory and synchronises its stream before it returns,
 * nb_generator_destroy frees (after a device synchronisation).  nb_generator_forward only enqueues, on one stream and as one
 * chain of launches: after one eager call at a batch size (it sets per-kernel attributes the first time) it can be captured into
 * a hipGraph.  One handle runs one forward at a time (the workspaces belong to the handle): for concurrent forwards create one
 * handle per stream.  The query functions (param / layer tables) make no HIP call and work without a GPU. */

typedef struct NbGeneratorConfig {   /* config.GeneratorConfig */
    int32_t z_dim, c_dim, w_dim;      /* c_dim must be 0; z_dim, w_dim <= 512 */
    int32_t img_resolution;           /* power of two >= 4 */
    int32_t mapping_layers;
    float   mapping_lr_multiplier;
    int32_t channel_base, channel_max;
    float   conv_clamp;               /* < 0 = None */
    int32_t num_geom;                 /* geometry features, 0..4 */
    int32_t geom_channels[4];
    int32_t geom_resolutions[4];      /* all 0 = the default (R/8, R/4), which needs num_geom == 2 */
} NbGeneratorConfig;

typedef struct NbGeneratorLayerInfo { /* config.LayerSpec */
    int32_t block_res, up, in_channels, out_channels, geom_channels, w_index;
} NbGeneratorLayerInfo;

#define NB_CONV_F32 0                 /* conv_mode: "f32", "h3", "f8" (the parity modes); "f6", "f16" -> NB_EUNSUPPORTED */
#define NB_CONV_H3  1
#define NB_CONV_F8  2
#define NB_CONV_F6  3
#define NB_CONV_F16 4
#define NB_NOISE_CONST  0             /* noise_mode */
#define NB_NOISE_NONE   1
#define NB_NOISE_RANDOM 2             /* -> NB_EUNSUPPORTED (torch's global generator has no counterpart here) */
/*      NB_NOISE_SEEDED 3                reproducible random noise: nb_noise_seeded_f32 (defined there) */
#define NB_RENDER_CLEAR 0             /* render_mode: alpha = u + v / 1 (nb_torgb_triad_f32) */
#define NB_RENDER_FULL  1

typedef struct NbGenerator NbGenerator;

/* Parameters = the state-dict tensors in the order of weights.random_state_dict: count, then name / shape of entry i
 * (ndim 0 = a scalar; shape[] entries beyond ndim are 0). */
int nb_generator_param_count(const NbGeneratorConfig* cfg);
int nb_generator_param_info(const NbGeneratorConfig* cfg, int i, char* name, int len, int64_t shape[4], int* ndim);
/* Layers = config.GeneratorConfig.layers in execution order (returns their count; *num_ws may be NULL). */
int nb_generator_layer_count(const NbGeneratorConfig* cfg, int* num_ws);
int nb_generator_layer_info(const NbGeneratorConfig* cfg, int i, char* name, int len, NbGeneratorLayerInfo* info);

/* params_dev[i]: device fp32 tensor of parameter i (contiguous, shapes as nb_generator_param_info).  Copies and packs what the
 * forward needs, allocates every workspace for batches up to n_max and synchronises `stream`: the caller may free params_dev
 * afterwards.  The current device is the generator's device. */
int nb_generator_create(const NbGeneratorConfig* cfg, const void* const* params_dev, int conv_mode, int n_max, void* stream,
                        NbGenerator** out);
int nb_generator_destroy(NbGenerator* gen);

typedef struct NbGeneratorInputs {
    const float* z;                   /* [n, z_dim], or NULL with ws given */
    const float* ws;                  /* [n, num_ws, w_dim], or NULL with z given (exactly one of the two) */
    float truncation_psi;             /* z only: ws[:, :cutoff] = w_avg + psi (ws - w_avg); 1 = off (ws input: must be 1) */
    int32_t truncation_cutoff;        /* < 0 = every ws */
    const float* geom[4];             /* geometry features [n, geom_channels[k], res_k, res_k] fp32, one per feature */
    const int64_t* positions;         /* [n, 2] (y, x) patch positions, or NULL (no positional noise shift) */
    int32_t noise_mode;               /* NB_NOISE_CONST / NB_NOISE_NONE / NB_NOISE_SEEDED */
    int32_t render_mode;              /* NB_RENDER_CLEAR / NB_RENDER_FULL */
    const float* user_colors;         /* [n, 3, 3] or NULL; NaN entries = the style's own colour */
    const float* sfactor;             /* [n] or NULL */
    /* NB_NOISE_SEEDED: every layer that runs gets nb_noise_seeded_f32's image of (noise_seed, noise_offset + sample index, its
     * absolute layer index), written by one launch in front of the layers (whole, geometry and staged passes alike; positions are
     * ignored).  noise_state: NULL, or a device pointer to {seed, offset} that replaces the two by-value fields -- the form for a
     * captured graph.  Other modes ignore the three. */
    uint64_t noise_seed, noise_offset;
    const uint64_t* noise_state;
} NbGeneratorInputs;

typedef struct NbGeneratorOutputs {   /* device pointers; NULL = not wanted */
    uint8_t* rgba_u8;                 /* [n, R, R, 4] */
    float* rgba;                      /* [n, 4, R, R] */
    float* img;                       /* [n, 3, R, R] */
    float* uvs;                       /* [n, 3, R, R] */
    float* colors;                    /* [n, 3, 3] */
} NbGeneratorOutputs;

/* One forward pass of batch n <= n_max on `stream` (enqueue only; no allocation, no synchronisation, no blocking copy).
 * n out of range, another current device than the generator's, a missing z / ws / geometry feature: NB_EINVAL, nothing
 * enqueued.  noise_mode random: NB_EUNSUPPORTED.  Device pointers of the inputs and outputs must stay valid until the work
 * has run. */
int nb_generator_forward(NbGenerator* gen, const NbGeneratorInputs* in, const NbGeneratorOutputs* out, int n, void* stream);

/* The kernel every layer's launch will run at batch n: "layer name=kernel name" lines (the strings SynthesisNetwork.layer_kernels
 * records), the ToRGB's line included: the last conv's kernel when it is fused there, else torgb_triad_kernel.  Host only. */
int nb_generator_describe(NbGenerator* gen, int n, char* buf, int len);

/* ---- the geometry encoder behind the generator handle: stroke patches -> RGBA in one chain ------------------------------------
 * encoder.HipGeometryEncoder (AutoEncoder.encode(res=[0, 1]) of the reference's `sauto` encoder) attached to a generator whose
 * geometry layout is the encoder's: two features, 16 channels at R/8 and 256 at R/4; R = 32, 64 or a multiple of 128.  The encoder's
 * operand formats, fused stem and hand-off of feature 1 into its consumer's operand tensor are those of the package's Python pass on
 * encoder.LazyGeometry (with TileOps' rule: f8 operands between the encoder's layers iff the generator is NB_CONV_F8), and so are the
 * results, bit for bit. */

/* Encoder parameters: the tensors AutoEncoder.encode(res=[0, 1]) reads, in encoder.ENCODER_STATE_SHAPES order without
 * num_batches_tracked: encoder.model.{0..5}.conv.{0,1}.* and decoder.model.0.conv.conv.{0,1}.* (42 entries).  Host only. */
int nb_encoder_param_count(void);
int nb_encoder_param_info(int i, char* name, int len, int64_t shape[4], int* ndim);

#define NB_GEOM_PREPROC_NONE       0   /* preproc_type None / "none" */
#define NB_GEOM_PREPROC_M11INVERSE 1   /* "-11inverse": (1 - x) * 2 - 1 */
#define NB_GEOM_PREPROC_INVERSE    2   /* "inverse": 1 - x */

/* NB_OK if an encoder with this preproc can be attached to a generator of this configuration, else NB_EINVAL with a message.
 * Host only (nb_generator_attach_encoder applies the same rules first). */
int nb_generator_encoder_check(const NbGeneratorConfig* cfg, int preproc);

/* Folds BatchNorm (float64, rounded to fp32), packs the weights on the device (hi/lo f16, and the f8 format for an NB_CONV_F8 generator),
 * allocates the encoder workspaces for every batch up to the handle's n_max and synchronises `stream`: the caller may then free
 * enc_params_dev (device fp32 tensors, shapes as nb_encoder_param_info).  A second call replaces the first. */
int nb_generator_attach_encoder(NbGenerator* gen, const void* const* enc_params_dev, int preproc, void* stream);

/* nb_generator_forward from stroke patches: geom [n, 1, R, R] fp32 (1 = background, what nb_geom_tiles_f32 writes); in->geom[] must
 * all be NULL.  Mapping / styles / noise, the encoder, the synthesis layers and the fused ToRGB, enqueued as one chain on `stream`
 * (no allocation): capturable into a hipGraph after one eager call at the batch size.  No encoder attached, a geometry feature given,
 * NULL geom, or any input nb_generator_forward rejects: NB_EINVAL (NB_EUNSUPPORTED for random noise), nothing enqueued. */
int nb_generator_forward_geom(NbGenerator* gen, const NbGeneratorInputs* in, const float* geom, const NbGeneratorOutputs* out, int n,
                              void* stream);

/* ---- staged passes: the generator split around the feature-canvas blend --------------------------------------------------------
 * The reference blends a tile's features with the feature canvas INSIDE its one synthesis pass (networks_modified.py:168-222:
 * BlendedFeatures.blend, forger/train/stitching.py:24-25, on the output of the blending block).  Here the blend of all tiles is one
 * launch (nb_canvas_replay_f32) between two batched generator passes, so the pass is cut at the blending block:
 *   head (stop_res):   mapping ... block stop_res; the block's last layer writes its fp32 output, before blending, into features_out.
 *                      No ToRGB runs: every pointer of NbGeneratorOutputs must be NULL (out itself may be NULL).  Styles are
 *                      computed for every layer, noise images only for the layers that run.
 *   tail (resume_res): the pass starts behind block resume_res from features_in (the blended features) and ends with the ToRGB and
 *                      compositing; if resume_res is a geometry resolution that feature joins features_in as the next block's input.
 *                      resume_res = R runs nothing but nb_torgb_triad_f32.  Noise images only for the blocks behind resume_res.
 * Exactly one of stop_res / resume_res is non-zero, a block resolution 4..R.  geom: stroke patches for the attached encoder (as
 * nb_generator_forward_geom; in->geom[] then all NULL) or NULL with the features in in->geom[].  A tail needs only the features at
 * resolutions >= resume_res; when it needs none, geom and in->geom[] are ignored and the encoder does not run.  The two passes of a
 * tile batch are SynthesisNetwork's `_stop_after` / `_resume` passes of the package (painting.PaintingHelper._schedule), bit for bit.
 * Enqueue only, one stream, no allocation: capturable into a hipGraph after one eager call at the batch size and stage.  A bad
 * stage, a NULL features pointer, a missing feature or any input nb_generator_forward rejects: NB_EINVAL (NB_EUNSUPPORTED for random
 * noise), nothing enqueued. */
typedef struct NbGeneratorStage {
    int32_t stop_res;          /* 0, or a block resolution 4..R: the pass ends after block stop_res */
    int32_t resume_res;        /* 0, or a block resolution 4..R: the pass starts after block resume_res */
    float* features_out;       /* stop_res: [n, channels(stop_res), stop_res, stop_res] fp32, the block's output before blending */
    const float* features_in;  /* resume_res: [n, channels(resume_res), resume_res, resume_res] fp32 (blended) */
} NbGeneratorStage;
int nb_generator_forward_staged(NbGenerator* gen, const NbGeneratorInputs* in, const float* geom, const NbGeneratorStage* stage,
                                const NbGeneratorOutputs* out, int n, void* stream);

/* nb_generator_describe for a staged pass: the lines of the layers the pass runs (the strings SynthesisNetwork.layer_kernels
 * records for them), and for a tail the ToRGB's line.  Host only. */
int nb_generator_describe_staged(NbGenerator* gen, int n, int stop_res, int resume_res, char* buf, int len);

/* ---- brush noise sets: a projected brush's noise buffers as a device object -----------------------------------------------------
 * A projected brush is a W+ code AND a noise_const replacement for every synthesis layer, optimised together with it (the
 * reference's brush libraries store {'w': ws, 'noise': {...}}, forger/ui/library.py:146-202; its engine renders with
 * G.forward_pre_mapped(ws, ..., noise_buffers=...), forger/ui/brush.py:746-754; the buffers replace noise_const before the
 * positional shift, networks.py:372-382).  A noise set holds, per layer, that replacement and its transpose at device addresses that
 * never change, so the pass that reads it is the ordinary planned pass: in-kernel noise of the large kernels (which read the
 * transpose, NbNoiseSrc) and the fused styles + noise launch of small batches included. */

/* One launch that writes every layer of a set: dst = a (b == NULL) or a * wa + b * wb, and dst_t = dst transposed.  The lerp is two
 * rounded fp32 products and one rounded fp32 sum, never an FMA: what `a * alpha + b * (1 - alpha)` gives on float32 arrays
 * (formats.WBrushLibrary.set_interpolated_style); the caller rounds wa = (float)alpha and wb = (float)(1 - alpha) from double.
 * layers_host is a HOST array of at most NB_PLAN_MAX_LAYERS entries, passed to the kernel by value; its pointers are device
 * pointers to fp32 [res, res] images (4-byte alignment suffices), res a power of two >= 4.  dst may be a (a reload in place); dst_t
 * must alias neither a nor b nor dst.  Enqueue only.  NULL layers_host, n_layers outside [1, NB_PLAN_MAX_LAYERS], a NULL a / dst /
 * dst_t or a bad res: NB_EINVAL, nothing enqueued. */
typedef struct NbBrushNoiseLayer {
    const float* a;            /* [res, res] */
    const float* b;            /* [res, res] or NULL */
    float* dst;                /* [res, res] = a (b == NULL) | a * wa + b * wb */
    float* dst_t;              /* [res, res] = dst transposed */
    int32_t res, pad;
} NbBrushNoiseLayer;
int nb_brush_noise_build_f32(const NbBrushNoiseLayer* layers_host, int n_layers, float wa, float wb, void* stream);

/* The set of a generator handle.
 *   create   allocates the set (sum over the layers of 2 res^2 floats), fills it with the checkpoint's noise_const -- an unloaded set
 *            renders exactly like no set --, uploads copies of every layer table the handle keeps with noise_const pointing into the
 *            set, and synchronises `stream` (as nb_generator_create does).  The current device must be the generator's.
 *   load     a_dev[i] / b_dev[i]: device fp32 [res_i, res_i] buffers in the order of nb_generator_layer_info; a NULL entry stands for
 *            the checkpoint's buffer of that layer, b_dev itself may be NULL.  With b_dev the set becomes a * alpha + b * (1 - alpha)
 *            (nb_brush_noise_build_f32 with wa = (float)alpha, wb = (float)(1 - (double)alpha)), else a.  One launch, enqueue only,
 *            capturable; the buffers must stay valid until it has run.
 *   bind     host state only: every later nb_generator_forward, _forward_geom and _forward_staged of the handle with NB_NOISE_CONST
 *            reads noise_const from the set's tables and hands the set's transposes to the kernels that compute their noise
 *            themselves.  The plan does not change (nb_generator_describe gives the same lines).  The other noise modes ignore the
 *            binding.  bn = NULL: back to the checkpoint's noise.  A set of another generator: NB_EINVAL.
 *   destroy  unbinds the set if it is bound, synchronises the device and frees it.  Destroy a generator's sets before the generator.
 * Graphs: the set's addresses never change, so a graph captured while a set is bound renders whatever nb_brush_noise_load wrote
 * last: switching brushes costs one launch (in stream order with the replays) and no recapture. */
typedef struct NbBrushNoise NbBrushNoise;
int nb_brush_noise_create(NbGenerator* gen, void* stream, NbBrushNoise** out);
int nb_brush_noise_load(NbBrushNoise* bn, const float* const* a_dev, const float* const* b_dev, float alpha, void* stream);
int nb_generator_bind_brush_noise(NbGenerator* gen, NbBrushNoise* bn);
int nb_brush_noise_destroy(NbBrushNoise* bn);

/* ---- the per-batch layer plan (host only: no HIP call, works without a GPU) ------------------------------------------------
 * Every kernel decision of one synthesis pass at batch n: which kernel each layer runs, its operand formats, the operand hand-off,
 * the fused ToRGB, in-kernel noise, the styles / noise launches and the early geometry packs.  The package's Python pass
 * (SynthesisNetwork) and nb_generator_forward both follow it. */

#define NB_PLAN_MAX_LAYERS 24         /* 2 log2(R / 4) + 1 layers: 21 at R = 4096 */
#define NB_PLAN_POS_NONE 0            /* NbPlanOptions.noise_positions */
#define NB_PLAN_POS_INT  1            /* constant noise shifted by integer patch positions */
#define NB_PLAN_POS_NORM 2            /* ... by normalised positions */
#define NB_KERNEL_F32      0          /* NbLayerPlan.kind: exact-fp32 kernels (nb_modconv3x3_f32) */
#define NB_KERNEL_SMALL_H3 1          /* split-f16 small-image kernels (nb_modconv3x3_up{1,2}_small_h3) */
#define NB_KERNEL_LARGE_H3 2          /* split-f16 large-tile kernels (nb_modconv3x3_up{1,2}_h3_ex) */
#define NB_PACK_H3     1              /* NbLayerPlan.packs: nb_pack_conv_weight_h3 */
#define NB_PACK_F8     2              /* the "f8" weight format */
#define NB_PACK_F6     4              /* the "f6" weight format */
#define NB_PACK_H3_UP2 8              /* the four FIR-folded up=2 phase kernels (nb_pack_conv_weight_h3_up2_dev) */

typedef struct NbPlanOptions {
    int32_t conv_mode;                /* NB_CONV_* */
    /* a layer takes the large split-f16 kernels from h3_min_pixels output pixels per batch and from batch h3_min_batch; the
     * up=2 layers with 16x16 / 8x8 inputs (quad tiles that cover a sample with few workgroups) from these batches */
    int32_t h3_min_pixels, h3_min_batch, h3_up2_w16_min_batch, h3_up2_w8_min_batch;
    /* switches (0 / 1): small-image split-f16 kernels; operand hand-off between large layers; early geometry packs; ToRGB fused
     * into a large last layer; in-kernel noise of the large layers; positions normalised once per batch; the latency-oriented
     * styles launch (where the shapes allow it) */
    int32_t small_h3, h2_handoff, early_geom_pack, fuse_torgb, noise_in_kernel, positions_once, styles_fast;
    /* the pass: NB_PLAN_POS_* (constant noise with positions; NONE for constant noise without them or other noise modes);
     * noise_overrides = per-call noise_const replacements; block resolutions (bit log2(res)) whose fp32 output the caller taps
     * (feature taps, a pass that stops after the block) or blends; resume_res = the pass starts after this block (0 = none) */
    int32_t noise_positions, noise_overrides, tap_mask, blend_mask, resume_res;
} NbPlanOptions;

typedef struct NbLayerPlan {
    char kernel[64];                  /* the kernel's name (SynthesisNetwork.layer_kernels, nb_generator_describe) */
    int32_t kind;                     /* NB_KERNEL_* */
    int32_t in_fmt;                   /* large: operand format of the input, 0 H2, 1 f8, 2 f6 (else 0) */
    int32_t kernel_fmt;               /* large: the kernel's in_fmt argument (3 = f8 operands, hi x hi products only: "f16") */
    int32_t out_fmt;                  /* handoff: the operand format the layer writes for the next one (else 0) */
    int32_t handoff;                  /* writes the next layer's operand input instead of fp32 output */
    int32_t fused_torgb;              /* the ToRGB + compositing run in this layer's epilogue */
    int32_t noise_in_kernel;          /* computes its shifted noise itself (NbNoiseSrc) */
    int32_t packs;                    /* NB_PACK_* weight forms the layer's launches may need (at any batch) */
} NbLayerPlan;

typedef struct NbGeomPlan {
    int32_t consumer;                 /* layer index of the consumer, b{2 res}.conv0 (-1: none, the feature is at R) */
    int32_t early_pack;               /* packed into the consumer's operands at the start of the pass */
    int32_t encoder_handoff;          /* the encoder may write it into the consumer's operands */
    int32_t fmt;                      /* the operand format of either (else 0) */
} NbGeomPlan;

typedef struct NbPassPlan {
    int32_t num_layers, num_geom;
    int32_t inkernel_from;            /* first layer from which every layer computes its noise itself (-1: none) */
    int32_t styles_fast;              /* nb_styles_fast_f32 (else nb_styles_f32) */
    int32_t styles_noise;             /* styles and noise images in one launch (nb_styles_noise_f32) */
    int32_t positions_once;           /* integer positions normalised once per batch (nb_norm_positions_f32) */
    NbLayerPlan layers[NB_PLAN_MAX_LAYERS];
    NbGeomPlan geom[4];
} NbPassPlan;

/* Today's defaults: the thresholds and switches both callers use, conv_mode NB_CONV_F8, a pass without positions. */
int nb_plan_options_default(NbPlanOptions* opts);
/* The plan of one pass at batch n (1 <= n <= 65535).  f6 / f16 are planned too. */
int nb_synthesis_plan(const NbGeneratorConfig* cfg, const NbPlanOptions* opts, int n, NbPassPlan* out);

/* ---- box calibration (csrc/nb_calib.hip; measurement infrastructure, not on the generator's path) -----------------
 * A registers-only loop of back-to-back v_mfma_f32_32x32x16_f16 on random operands, one wave per SIMD on every CU of the current
 * device, for about target_ms (blocking).  *tflops = the dense f16 matrix rate this device sustains, *ms = duration of the measured
 * launch, *clock_mhz = median in-kernel shader clock during it (may be NULL).  MI355X boards differ by several percent in the
 * clock they hold under matrix load; bench.py reports the figure beside its own (box_calibration, roofline.frac_of_sustained).
 * The reference has no counterpart (forger/util/timer.py:11-32 is its only timer). */
int nb_calibrate_mfma_f16(double target_ms, double* tflops, double* ms, double* clock_mhz, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NEUBE_HIP_H */
