/*
 * robustart_hip.h -- C-ABI of the MI355X (gfx950) hot path of RobustART's AddNoise:
 * ImageNet-C corruption kernels, adversarial step kernels and the eval-mode
 * ResNet-50 forward / backward-to-input engine.
 *
 * The reference (DIG-Beihang/RobustART) is pure Python and has no FFI of its own; this
 * header is the boundary a maintainer would bind with ctypes.  Each
 * entry point cites the reference function it replaces (paths relative to
 * RobustART/noise/utils/ unless stated).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HBM) unless its name ends in _host;
 *  - the library never allocates or frees caller memory; scratch comes from the caller's
 *    `workspace` (size from the matching *_workspace_bytes query);
 *  - all work is enqueued on `stream` (a hipStream_t); no hidden device synchronisation;
 *  - return value: 0 = RART_OK, otherwise an rart_status; rart_last_error_string() gives
 *    the thread-local message.  Nothing throws across the boundary or calls exit();
 *  - randomness is counter based: a draw is a pure function of
 *    (seed, global sample index = sample_offset + i, element index), independent of launch
 *    geometry and of how samples are sharded over GPUs.  When `injected` is non-NULL the
 *    kernels consume the caller's draws instead (parity mode, fp64 where the reference is
 *    fp64) -- layouts are listed per corruption below.
 */
#ifndef ROBUSTART_HIP_H
#define ROBUSTART_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* rart_stream_t; /* hipStream_t */

typedef enum rart_status {
  RART_OK = 0,
  RART_ERR_INVALID = 1,     /* bad argument (null pointer, severity outside 1..5, unknown id ...) */
  RART_ERR_UNSUPPORTED = 2, /* valid request the library does not implement (e.g. a conv geometry no kernel instance covers) */
  RART_ERR_WORKSPACE = 3,   /* workspace missing or too small */
  RART_ERR_HIP = 4          /* a HIP runtime call failed */
} rart_status;

/* corruption ids == index into corruption_tuple (imagenet_c/__init__.py:5-8) */
enum {
  RART_GAUSSIAN_NOISE = 0, RART_SHOT_NOISE = 1, RART_IMPULSE_NOISE = 2, RART_DEFOCUS_BLUR = 3,
  RART_GLASS_BLUR = 4, RART_MOTION_BLUR = 5, RART_ZOOM_BLUR = 6, RART_SNOW = 7, RART_FROST = 8,
  RART_FOG = 9, RART_BRIGHTNESS = 10, RART_CONTRAST = 11, RART_ELASTIC_TRANSFORM = 12,
  RART_PIXELATE = 13, RART_JPEG_COMPRESSION = 14, RART_SPECKLE_NOISE = 15, RART_GAUSSIAN_BLUR = 16,
  RART_SPATTER = 17, RART_SATURATE = 18, RART_NUM_CORRUPTIONS = 19
};

/* ABI version of THIS header.  Bumped whenever a struct layout or a signature changes (round 3 -> 4: rart_conv_desc grew
 * its tap arrays from 16 to 32 entries and gained dst_pair_off / res_pair_off; several attack entries gained a per-row
 * sample-index pointer; round 4 -> 5: rart_stencil_fixed_point_info added).  A caller compiled against another header must refuse to run:
 * compare with rart_version(). */
#define RART_ABI_VERSION 110
int rart_version(void);
const char* rart_last_error_string(void);
/* name of corruption id (static string), NULL if out of range */
const char* rart_corruption_name(int corruption_id);

/* ---------------------------------------------------------------------------------------
 * ImageNet-C corruptions.  Replaces corrupt() + the per-image Python loop of
 * add_noise_for_imagenet_c (add_noise_utils.py:22-31, imagenet_c/__init__.py:13-35,
 * imagenet_c/corruptions.py:122-424).
 *
 * in / out : uint8 NHWC (n, h, w, 3); may alias (in-place, as the reference mutates its input).
 *            Corruptions the reference hard-codes to 224x224 (glass_blur, fog, frost, snow,
 *            pixelate, elastic_transform) require h == w == 224 here too.
 * severity : 1..5.
 * injected : NULL (native counter-based RNG) or an array of device pointers holding what
 *            np.random returned inside the reference function, per image, C order:
 *   gaussian_noise, speckle_noise : [0] double noise[n][h][w][3]   (np.random.normal(scale=c))
 *   shot_noise                    : [0] int32  counts[n][h][w][3]  (np.random.poisson)
 *   impulse_noise                 : [0] uint8  code[n][h][w][3]    (0 keep, 1 salt, 2 pepper)
 *   glass_blur                    : [0] int8   dxdy[n][iters][224-2d][224-2d][2]   (every value in [-d, d): numpy's randint(-d, d);
 *                                       the overlapped copy chain packs dx + d, dy + d into nibbles -- the Python entry refuses others)
 *   motion_blur                   : [0] double angle[n]
 *   snow                          : [0] double layer[n][224][224]  [1] double angle[n]
 *   frost                         : [0] uint8  texture_crop[n][224][224][3]  (REQUIRED always: the
 *                                       reference's frost photos are not in its repository)
 *   fog                           : [0] double uniform[n][65535]   (plasma_fractal draws, call order)
 *   elastic_transform             : [0] float  jitter[n][3][2]  [1] double field_x[n][224][224]
 *                                   [2] double field_y[n][224][224]
 *                                   (severities 1-2: the field filter runs as fp64 matrix products against the folded reflect-filter
 *                                   matrix, resident on the device after the first call -- not scipy's summation order: the fields
 *                                   differ in the last bits, the images stay within the corruption's stated tolerance (<= 1 LSB on <= 1e-4
 *                                   of the pixels) and are NOT guaranteed bit-identical to the ordered kernels; RART_ELASTIC_ORDERED=1 in the
 *                                   environment selects the ordered, bit-exact kernels.  The first severity-1 / 2 call per device
 *                                   allocates: keep it outside stream capture)
 *   spatter                       : [0] double layer[n][224][224]
 *   others                        : ignored
 * workspace: rart_corrupt_workspace_bytes(...) bytes, 256-byte aligned.
 * ------------------------------------------------------------------------------------- */
size_t rart_corrupt_workspace_bytes(int corruption_id, int severity, int n, int h, int w);

int rart_corrupt_u8(const uint8_t* in, uint8_t* out, int n, int h, int w,
                    int corruption_id, int severity,
                    uint64_t seed, uint64_t sample_offset,
                    const void* const* injected_host_array, int n_injected,
                    void* workspace, size_t workspace_bytes, rart_stream_t stream);

/* gaussian_noise / speckle_noise at ns <= 8 (severity, seed) pairs of ONE source batch in one launch: every 1 KiB chunk is read once and
 * written ns times, each output with its own field.  outs[i] is bit-identical to rart_corrupt_u8(in, outs[i], n, h, w, corruption_id,
 * severities[i], seeds[i], sample_offset, NULL, 0, ...) with the native matrix-core generator.  ImageNet-C generation corrupts every
 * image at five severities (imagenet_c/__init__.py:13-35 once per (image, severity)): five launches move 10 x the batch through HBM,
 * this one 6 x.  outs: HOST array of ns device pointers.  RART_ERR_UNSUPPORTED unless h*w*3 % 1024 == 0 with 16-byte aligned
 * buffers and the matrix-core generator selected (callers then issue ns rart_corrupt_u8 calls). */
int rart_noise_multi_u8(const uint8_t* in, uint8_t* const* outs, int ns, int n, int h, int w, int corruption_id, const int* severities,
                        const uint64_t* seeds, uint64_t sample_offset, rart_stream_t stream);

/* frost from device-resident photographs (round 5).  The reference (imagenet_c/corruptions.py:249-266) opens one of its frost photographs
 * per image -- randint(5) over a six-entry list -- crops 224 x 224 at a random origin and blends; the photographs are not in its repository, so
 * the caller registers them (robustart_amd.noise.imagenet_c.set_frost_textures) and they live on the device as one stack
 * uint8 [k_tex][sh][sw][3] (each padded to the common size; dims_host: host int[2 k_tex] = height, width of each).  The texture index and the
 * crop origin of image i are the counter generator's uniforms of streams 8, 9, 10 at sample sample_offset + i, drawn in the kernel, which reads
 * the crop in place: bit-identical to rart_corrupt_u8(RART_FROST) with those crops injected, without the gather (n x 150 528 B written and
 * read back).  h = w = 224 only, as the reference; in / out 16-byte aligned.  in == out allowed. */
int rart_frost_textures_u8(const uint8_t* in, uint8_t* out, int n, int h, int w, int severity, const uint8_t* stack, int k_tex, int sh, int sw,
                           const int* dims_host, uint64_t seed, uint64_t sample_offset, rart_stream_t stream);

/* Host-only introspection of the fixed-point tables behind the matrix-core stencil paths (round 5; no GPU needed: the "-m 'not gpu'"
 * tests check the tables against the oracle's weights).  defocus_blur (corruptions.py:187-198: 17 x 17 disks, 21 x 21 at severity 5) runs as an
 * exact 2-D integer filter, gaussian_blur (corruptions.py:162-166) and glass_blur's two blurs (corruptions.py:169-184) as an exact
 * separable one: W = round(w 2^frac_bits) split into four signed base-256 digits laid out as v_mfma_i32_16x16x64_i8 A-operand
 * fragments -- fragment (step j, digit d), lane (m = lane & 15, g = lane >> 4), byte i:
 *   kind 1 (2-D):       kernel row 2 j + (g >> 1), window column 16 (g & 1) + i, tap b = column - m; rows m >= 33 - ksize are zero
 *                       (n_steps = (ksize + 1) / 2: 9 for 17 x 17, 11 for 21 x 21 whose row blocks hold 12 outputs)
 *   kind 2 (separable): tap t = 16 g + i - m of the 1-D kernel                                            (n_steps = 1)
 * An output whose fixed-point value lies within `band` units (of 2^-out_frac_bits of an output step) of an integer is recomputed in the
 * reference's fp64 order.  blur_index: 0 for defocus_blur / gaussian_blur; glass_blur has one sigma, index 0.
 * frags: NULL or a HOST buffer of n_steps * 4 * 64 * 16 bytes.  Returns RART_ERR_UNSUPPORTED (kind 0) where the fp64 kernels run. */
typedef struct rart_fixed_point_info {
  int kind, ksize, n_steps, frac_bits, out_frac_bits;
  long long corr, band;
  double max_abs_weight_error;      /* max |W / 2^frac_bits - w| over the taps */
  double sum_abs_weight_error;
} rart_fixed_point_info;
int rart_stencil_fixed_point_info(int corruption_id, int severity, rart_fixed_point_info* info, unsigned char* frags, size_t frags_bytes);

/* ImageNet-S resize operators (imagenet_s_gen.py:19-34,127-166): Pillow's Image.resize((resize_w, resize_h), filter) on
 * uint8 NHWC images followed by a crop, bit-exact with Pillow (Resample.c 22-bit fixed point; Geometry.c for
 * NEAREST).  filter = PIL.Image constant: 0 nearest, 1 bilinear, 2 bicubic, 3 box, 4 hamming, 5 lanczos.
 * out: uint8 [n][crop_h][crop_w][3] = resized[crop_y : crop_y+crop_h, crop_x : crop_x+crop_w]. */
size_t rart_pil_resize_workspace_bytes(int n, int h, int w, int resize_h, int resize_w, int filter, int crop_y, int crop_x,
                                       int crop_h, int crop_w);
int rart_pil_resize_u8(const uint8_t* in, uint8_t* out, int n, int h, int w, int resize_h, int resize_w, int filter,
                       int crop_y, int crop_x, int crop_h, int crop_w, void* workspace, size_t workspace_bytes,
                       rart_stream_t stream);
/* The 'opencv-*' ImageNet-S resize operators (imagenet_s_gen.py:27-33,138-146): cv2.resize(img, (resize_w, resize_h),
 * interpolation) on uint8 NHWC images followed by a crop.  interpolation = cv2 constant: 0 INTER_NEAREST, 1 INTER_LINEAR,
 * 2 INTER_CUBIC, 3 INTER_AREA, 4 INTER_LANCZOS4.  Restates opencv/modules/imgproc/src/resize.cpp (4.x) -- OpenCV is an
 * unpinned dependency absent from the build container: parity unpinned.  out: uint8 [n][crop_h][crop_w][3]. */
size_t rart_cv_resize_workspace_bytes(int n, int h, int w, int resize_h, int resize_w, int interpolation, int crop_y,
                                      int crop_x, int crop_h, int crop_w);
int rart_cv_resize_u8(const uint8_t* in, uint8_t* out, int n, int h, int w, int resize_h, int resize_w, int interpolation,
                      int crop_y, int crop_x, int crop_h, int crop_w, void* workspace, size_t workspace_bytes,
                      rart_stream_t stream);

/* uint8 NHWC -> ImageNet-normalised tensor for the model ((x/255 - mean)/std), i.e. the ToTensor +
 * Normalize step that follows AddNoise in the reference's eval pipeline
 * (exprs/exp/imagenet_c_loop_mini/config_vit_base.yaml:85-99).
 * out_dtype : 0 = fp32, 1 = bf16.   out_layout : 0 = NCHW, 1 = NHWC. */
int rart_u8_to_normalized(const uint8_t* in, void* out, int n, int h, int w,
                          int out_dtype, int out_layout, rart_stream_t stream);
/* x01 fp32 NCHW = u8 NHWC * (1 / 255) (bit-identical to torch's u8.permute(0, 3, 1, 2).float().div(255), which multiplies by the fp32
 * reciprocal of a scalar divisor): the hand-over from
 * the uint8 images of the corruption kernels / datasets to the attack tensors (fp32 NCHW in [0,1], adv/attack.py:20-23) in one kernel. */
int rart_u8_to_unit_f32_nchw(const uint8_t* in, float* out, int n, int h, int w, rart_stream_t stream);

/* Fill helpers exposing the library's counter-based generator (used by the parity tests to
 * replay the native noise field on the host oracle, and by the attack random starts).
 * stream_id selects an independent sub-stream (0..15). */
int rart_rng_uniform_u32(uint32_t* out, int n_samples, size_t elems_per_sample,
                         uint64_t seed, uint64_t sample_offset, int stream_id, rart_stream_t stream);
int rart_rng_normal_f32(float* out, int n_samples, size_t elems_per_sample,
                        uint64_t seed, uint64_t sample_offset, int stream_id, rart_stream_t stream);
/* Normal generator of gaussian_noise / speckle_noise: 1 (default) = matrix-core CLT generator (int8 MFMA
 * against a Hadamard matrix, one random byte per normal, cubic kurtosis correction) whenever a sample is a
 * whole number of 1 KiB chunks; 0 = Threefry + Box-Muller everywhere.  rart_rng_noise_field_f32 replays the
 * N(0,1) field those two corruptions use under the current setting. */
int rart_set_normal_generator(int kind);
/* Measurement aid of bench.py (hbm_roofline_gaussian_noise): a plain device copy of `bytes` (multiple of 16, 16-byte aligned buffers) --
 * variant 0: one 16-byte vector per lane, one wave per 1 KiB, the noise kernels' launch geometry; variant 1: a grid-stride loop over 1 024
 * workgroups.  What a kernel that only moves a launch's bytes reaches at that size is the ceiling the noise kernels are read against. */
int rart_copy_calibration(const void* in, void* out, size_t bytes, int variant, rart_stream_t stream);
int rart_get_normal_generator(void);
int rart_rng_noise_field_f32(float* out, int n_samples, size_t elems_per_sample, uint64_t seed,
                             uint64_t sample_offset, rart_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Adversarial step kernels (x, x0, g: fp32, batch-major, n_per_sample elements per sample,
 * values of x in [0,1] BEFORE normalisation, as in the reference).
 * ------------------------------------------------------------------------------------- */

/* Workspace size (bytes) that satisfies every attack entry point below for `batch` samples. */
size_t rart_attack_workspace_bytes(int batch);

/* x = clip(x0 + U(-eps, eps), lo, hi).  foolbox LinfPGD random start (adv/attack.py:20-23);
 * with clip_lo > clip_hi the clip is skipped = MIM start (Attacks/imfgsm_attack.py:73-74).
 * injected_u: NULL or fp32 U(-eps,eps) draws shaped like x. */
/* row_samples (here and in the entries below that take it): NULL, or int64 [batch] on the device -- the GLOBAL sample index of every
 * row.  Row b then draws at row_samples[b] instead of sample_offset + b: inside AutoAttack the sub-attacks receive the still-robust
 * SUBSET of a batch (autoattack.py:117-136), and with its rows' own indices the draws of a sample do not depend on which other
 * samples survived, i.e. on how the dataset is batched or sharded over GPUs. */
int rart_attack_init_linf(float* x, const float* x0, int batch, size_t n_per_sample, float eps,
                          float clip_lo, float clip_hi, uint64_t seed, uint64_t sample_offset, const int64_t* row_samples,
                          const float* injected_u, rart_stream_t stream);

/* x <- clip(x0 + clip(x + alpha*sign(g) - x0, -eps, eps), 0, 1): one fused PGD-Linf / FGSM step
 * (foolbox BaseGradientDescent.run, adv/attack.py:20-23,30-33). */
int rart_pgd_step_linf(float* x, const float* g, const float* x0, size_t n_elems,
                       float eps, float alpha, rart_stream_t stream);

/* PGD-L2 step (adv/attack.py:25-28): x += alpha*g/max(|g|_2,1e-12); delta *= min(1, eps/max(|delta|_2,1e-12));
 * clip [0,1].  workspace: rart_attack_workspace_bytes(batch). */
int rart_pgd_step_l2(float* x, const float* g, const float* x0, int batch, size_t n_per_sample,
                     float eps, float alpha, void* workspace, size_t workspace_bytes, rart_stream_t stream);
/* PGD-L1 step of ART's ProjectedGradientDescentPyTorch(norm=1) (adv/attack.py:44-49; ART is unpinned in the
 * reference's requirements.txt:25, this is the 1.x algorithm): x = clip(x + eps_step*g/(sum|g| + 1e-7), 0, 1);
 * x = x0 + (x - x0)*min(1, eps/(sum|x - x0| + 1e-7)).  workspace: rart_attack_workspace_bytes(batch). */
int rart_pgd_step_l1(float* x, const float* g, const float* x0, int batch, size_t n_per_sample, float eps, float eps_step,
                     void* workspace, size_t workspace_bytes, rart_stream_t stream);
/* ART random_sphere(norm=1) start: x = clip(x0 + r * s_i e_i / sum e, 0, 1), e ~ Exp(1), s = +-1, r = sqrt(U(0, eps^2)).
 * injected_signed_exp [batch][n] (s_i*e_i) and injected_radius [batch] replace the native draws (both or neither). */
int rart_random_start_l1(float* x, const float* x0, int batch, size_t n_per_sample, float eps, uint64_t seed,
                         uint64_t sample_offset, const int64_t* row_samples, const float* injected_signed_exp, const float* injected_radius,
                         void* workspace, size_t workspace_bytes, rart_stream_t stream);

/* MIM step (Attacks/imfgsm_attack.py:85-90): g/=mean|g| per sample; m = decay*m + g;
 * x = clip(x0 + clip(x + step*sign(m) - x0, +-eps), 0, 1).  workspace: rart_attack_workspace_bytes(batch). */
int rart_mim_step(float* x, float* momentum, const float* g, const float* x0, int batch,
                  size_t n_per_sample, float eps, float step_size, float decay,
                  void* workspace, size_t workspace_bytes, rart_stream_t stream);

/* APGD random start (Attacks/autoattack/autopgd_base.py:213-220,237):
 * x = clip(x0 + eps * t / (max|t| + 1e-12), 0, 1) for Linf, t ~ U(-1,1);
 * x = clip(x0 + eps * t / (|t|_2 + 1e-12), 0, 1) for L2, t ~ N(0,1).
 * norm: 0 = Linf, 1 = L2, 2 = L1 (normal draws divided by their L1 norm: the random start of FAB's restarts, fab_base.py:133-166, which
 * has the same x0 + r t / ||t|| form with r = eps / 2).  injected_t: NULL or the fp32 draws.  workspace: rart_attack_workspace_bytes(batch). */
int rart_apgd_init(float* x, const float* x0, int batch, size_t n_per_sample, int norm, float eps,
                   uint64_t seed, uint64_t sample_offset, const int64_t* row_samples, const float* injected_t,
                   void* workspace, size_t workspace_bytes, rart_stream_t stream);

/* APGD step with momentum and double projection (autopgd_base.py:327-348).
 * x_adv (in/out), x_adv_old (in/out: receives the pre-step x_adv), grad, x0; step_size: per-sample
 * fp32[batch]; a = 1.0 on the first iteration, 0.75 afterwards.  norm: 0 = Linf, 1 = L2.
 * workspace: rart_attack_workspace_bytes(batch) (L2 only). */
int rart_apgd_step(float* x_adv, float* x_adv_old, const float* grad, const float* x0,
                   const float* step_size, int batch, size_t n_per_sample, int norm, float eps, float a,
                   void* workspace, size_t workspace_bytes, rart_stream_t stream);

/* Square attack, Linf (Attacks/autoattack/square.py:228-258).  Start: x_best = clamp(x0 + eps*sign, 0, 1) with one
 * random sign per (image, channel, column); injected_sign: NULL or fp32 [batch][c][w] of +-1.
 * Proposal: x_new = clamp(min(max(x_best + delta, x0-eps), x0+eps), 0, 1), delta = 2*eps*sign_host[ch] inside the
 * s x s window at (vh, vw), shared by the whole batch like the reference. */
int rart_square_init_linf(float* x_best, const float* x0, int batch, int c, int h, int w, float eps, uint64_t seed,
                          uint64_t sample_offset, const int64_t* row_samples, const float* injected_sign, rart_stream_t stream);
/* out[b][j] = +1 / -1: the sign rows Square's L2 / L1 proposals multiply their windows with (square.py:343-345, 455-457), one per
 * (image, channel), from the counter generator on the device: bit 31 of the first Threefry word of counter (index_base + j, stream_id) of
 * row b's sample (the value noise/rng.py host_uniform(...) >= 0.5 gives).  Replaces a numpy draw + host-to-device copy per query.
 * rart_rng_normal_rows_f32: rart_rng_normal_f32 for explicit rows (out[b][:] = the field of sample row_samples[b]). */
int rart_rng_signs_f32(float* out, int batch, int n_per_row, uint64_t seed, uint64_t sample_offset, const int64_t* row_samples,
                       int stream_id, uint32_t index_base, rart_stream_t stream);
int rart_rng_normal_rows_f32(float* out, int batch, size_t elems, uint64_t seed, const int64_t* row_samples, int stream_id,
                             rart_stream_t stream);
int rart_square_propose_linf(float* x_new, const float* x_best, const float* x0, int batch, int c, int h, int w,
                             float eps, int vh, int vw, int s, const float* sign_host, rart_stream_t stream);

/* Expectation over transformation of APGD (autopgd_base.py:271-289, :367-384; AutoAttack version 'rand'): mode 0: acc += g over n fp32
 * elements; mode 1: acc /= divisor (the reference divides by float(eot_iter)). */
int rart_eot_accumulate(float* acc, const float* g, size_t n, int mode, float divisor, rart_stream_t stream);

/* Square attack, norm 2 = L2 / 1 = L1 (Attacks/autoattack/square.py:123-190, 296-530); all pointers are device pointers.
 * rart_square_init_lp: the start perturbation -- tiles of side s on a tiles_h x tiles_w grid from (sp, sp), tile t carries
 *   eta2[transposed[t]] (eta2 = [2][s*s]: eta(s) and its transpose, :172-190) times signs[t][image][channel] (+-1).  L2: out = the start
 *   point clamp(x0 + delta / (||delta||_2 + 1e-12) * eps, 0, 1); L1: out = delta (add rart_l1_project(x0, delta, eps (1 - 1e-6)), :425-426).
 * rart_square_propose_lp: one query -- window (vh, vw) of side s gets eta * signs[image][channel] + delta / (1e-12 + |delta|_window),
 *   rescaled to the budget left (:347-362 / :461-476), window (vh2, vw2) is cleared.  L2: out = the candidate point; L1: out = the new
 *   delta (then rart_l1_project, :483-484).  One workgroup per image; c <= 4. */
int rart_square_init_lp(float* out, const float* x0, int batch, int c, int h, int w, float eps, int norm, int s, int sp, int tiles_h,
                        int tiles_w, const float* eta2, const uint8_t* transposed, const float* signs, rart_stream_t stream);
int rart_square_propose_lp(float* out, const float* x_best, const float* x0, int batch, int c, int h, int w, float eps, int norm, int vh,
                           int vw, int vh2, int vw2, int s, const float* eta, const float* signs, rart_stream_t stream);

/* FAB, Linf (Attacks/autoattack/fab_projections.py:7-59, fab_base.py:168-245).
 * rart_fab_project_linf: per row r, the box-constrained Linf projection step d of points[r] onto {x: w[r].x = b[r]};
 *   rowmax_out[r] = max|d[r]| (nullable).  One workgroup per row, bisection on the monotone piecewise-linear
 *   constraint instead of the reference's argsort (same solution up to fp32 summation order).
 * rart_row_dot / rart_row_absmax_diff: per-row <a,b> and max|a-b|.
 * rart_fab_update: x1 = clamp((x1 + eta*d1)*(1-alpha[r]) + (x0 + eta*d2)*alpha[r], 0, 1).
 * rart_fab_backoff: rows with mask != 0: x1 = x0 + (x1 - x0)*beta. */
int rart_fab_project_linf(const float* points, const float* w, const float* b, float* d_out, float* rowmax_out, int rows,
                          size_t n, rart_stream_t stream);
/* rart_fab_project: the same step for norm 0 = Linf (projection_linf), 1 = L1 (projection_l1, fab_projections.py:120-166),
 * 2 = L2 (projection_l2, :62-117); rownorm_out[r] = ||d[r]||_norm (fab_base.py:194-203).  Sort-free: per row a bisection on the
 * bit pattern of the multiplier (L2) / of the |w| threshold (L1), then the exact solve of the segment.
 * rart_row_norm_diff: out[r] = ||a[r] - b[r]||_norm (fab_base.py:226-236). */
int rart_fab_project(const float* points, const float* w, const float* b, float* d_out, float* rownorm_out, int rows, size_t n,
                     int norm, rart_stream_t stream);
int rart_row_norm_diff(const float* a, const float* b, float* out, int rows, size_t n, int norm, rart_stream_t stream);
int rart_row_dot(const float* a, const float* b, float* out, int rows, size_t n, rart_stream_t stream);
int rart_row_absmax_diff(const float* a, const float* b, float* out, int rows, size_t n, rart_stream_t stream);
int rart_fab_update(float* x1, const float* x0, const float* d1, const float* d2, const float* alpha, int batch,
                    size_t n_per_sample, float eta, rart_stream_t stream);
int rart_fab_backoff(float* x1, const float* x0, const uint8_t* mask, int batch, size_t n_per_sample, float beta,
                     rart_stream_t stream);

/* ---- APGD with the L1 threat model (Attacks/autoattack/autopgd_base.py:19-83, 222-226, 351-364, 431-441) ----
 * rart_l1_project: the reference's L1_projection(x2 = x, y2 = y, eps1 = eps) for `rows` rows of n fp32 elements: delta with
 * ||y + delta||_1 <= eps and 0 <= x + y + delta <= 1.  out = delta (point_out = 0) or the projected point x + y + delta
 * (point_out = 1; clamp01 additionally clamps it to [0,1] as attack_single_run :237 does).  out may alias y.
 * rart_row_kth_abs: thr[r] = k[r]-th smallest (0-based, clamped to [0, n-1]) of |g[r][.]|, exact (radix select).
 * rart_apgd_l1_move: delta_u = x_adv + step_size[r] * sign(g * [|g| >= thr[r]]) / (count_r + 1e-10) - x0 (:355-360).
 * rart_row_count_diff: out[r] = #{i : a[r][i] != b[r][i]} as fp32 (L0_norm, other_utils.py:42-43). */
int rart_l1_project(const float* x, const float* y, float* out, int rows, size_t n, float eps, int point_out, int clamp01,
                    rart_stream_t stream);
int rart_row_kth_abs(const float* g, const int64_t* k, float* thr, int rows, size_t n, rart_stream_t stream);
int rart_apgd_l1_move(const float* x_adv, const float* grad, const float* x0, const float* thr, const float* step_size,
                      float* delta_u, int rows, size_t n, rart_stream_t stream);
int rart_row_count_diff(const float* a, const float* b, float* out, int rows, size_t n, rart_stream_t stream);

/* Per-sample select: dst[i] = src[i] where mask[i] != 0 (rows of n_per_sample floats).
 * The x_best / x_best_adv / grad_best bookkeeping of autopgd_base.py:389-406,426-427. */
int rart_select_rows(float* dst, const float* src, const uint8_t* mask, int batch, size_t n_per_sample,
                     rart_stream_t stream);

/* Row-wise losses on logits [batch][classes] fp32 (autopgd_base.py:198-204,599-604; CE of
 * foolbox / imfgsm_attack.py:83).  kind: 0 = CE, 1 = DLR, 2 = targeted DLR (y_target required),
 * 3 = margin z_y - max_{j != y} z_j (Attacks/autoattack/square.py:68-86),
 * 4 = FAB targeted difference -(z_y - z_t) (Attacks/autoattack/fab_pt.py:102-117).
 * loss_out[batch] (nullable), dlogits_out[batch][classes] = d(sum_i loss_i * scale)/dlogits (nullable),
 * pred_out[batch] int32 argmax (nullable). */
int rart_logit_loss(const float* logits, const int64_t* y, const int64_t* y_target, int batch, int classes,
                    int kind, float scale, float* loss_out, float* dlogits_out, int32_t* pred_out,
                    rart_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Eval-mode model engine (ResNet-50 forward / backward-to-input, the `f_model(x)` + autograd step
 * every attack iteration performs: adv/attack.py:21-22, autopgd_base.py:271-289,367-384,
 * imfgsm_attack.py:82-84; model definition: RobustART/model/__init__.py:1 -> absent submodule,
 * public ResNet-50 v1.5).  BatchNorm is folded into the conv weights/bias on the host (eval mode),
 * activations are bf16 NHWC, accumulation fp32.
 *
 * rart_conv_igemm_bf16: C[m][n] = sum_k A[m][k] * W[n][k] with A gathered from `src`:
 *   row m      <-> (image, oy, ox) over batch x grid_h x grid_w
 *   k          =  tap * k_per_tap + c,  tap t reads source pixel (oy*sy + tap_dy[t], ox*sx + tap_dx[t])
 *                 of the (src_h x src_w) image at element offset tap_src_off[t] + pixel*src_pix_stride + c
 *                 (zeros outside the image)
 *   W          :  bf16 [round_up(n_cols, 128 if n_cols > 64 else 64)][n_taps * k_per_tap], K contiguous
 *   destination:  element ((image*dst_h + oy*dst_sy + dst_oy)*dst_w + ox*dst_sx + dst_ox)*dst_pix_stride + n
 *   epilogue   :  v = acc + bias[n]; v += res[dst index]; if (mask) v = mask[dst index] > 0 ? v : 0;
 *                 if (flags & 1) v = max(v, 0); if (flags & 4) v = gelu(v); store bf16 (or fp32 if flags & 2).
 *                 flags & 8: `mask` holds a GELU pre-activation u instead and v = v * gelu'(u) (no sign masking).
 *                 `res` may alias `dst`.
 * Covers forward convs, backward-to-input of stride-1 convs, each input-parity class of a stride-2
 * conv's backward, the 7x7 stem on the padded 4-channel hi/lo image, and fully connected layers.
 * ------------------------------------------------------------------------------------- */
typedef struct rart_conv_desc {
  const void* src;
  const void* wgt;
  const float* bias;      /* fp32 [n_cols] or NULL */
  const void* res;        /* bf16, indexed like dst, or NULL */
  const void* mask;       /* bf16, indexed like dst, or NULL */
  void* dst;
  int32_t batch, grid_h, grid_w;
  int32_t src_h, src_w, src_pix_stride;
  int32_t k_per_tap, n_taps;
  int32_t sy, sx;
  int32_t tap_dy[32], tap_dx[32];
  int64_t tap_src_off[32];
  int32_t n_cols;
  int32_t dst_h, dst_w, dst_sy, dst_sx, dst_oy, dst_ox, dst_pix_stride;
  int32_t flags;          /* 1 = ReLU, 2 = fp32 output, 4 = exact GELU, 8 = GELU' of `mask`, 16 = `mask` is a 1-bit tensor,
                           * 32 = split-bf16 tensors (dst_pair_off / res_pair_off below), 64 = GELU with the pre-activation kept,
                           * 128 = the 1-bit `mask` (with 16) applies to the RESIDUAL instead of the result: dst = acc + res . [mask]
                           * (train engine: the skip gradient d_out . [out > 0] without materialising it) */
  /* batched problems (attention: one GEMM per (image, head)): problem z in [0, n_batched) splits into
   * zo = z / z_inner, zi = z % z_inner; zo*_z_outer + zi*_z_inner elements are added to src / wgt / dst (res and
   * mask follow dst).  n_batched <= 1 = a single problem.  wgt_row_stride: elements between consecutive weight
   * rows (0 = n_taps * k_per_tap), so K / V can be read in place from the fused qkv activation. */
  int32_t n_batched, z_inner, wgt_row_stride, reserved_;
  int64_t src_z_outer, src_z_inner, wgt_z_outer, wgt_z_inner, dst_z_outer, dst_z_inner;
  /* 1-bit-per-element sign tensors, indexed like dst (byte = element / 8, bit = element % 8): the eval engine's backward
   * needs activations only for their ReLU sign, so the forward GEMM writes (output > 0) here (nullable) and the backward
   * GEMM reads it through `mask` with flag 16 -- 1/16 of the bytes of a bf16 mask.  bf16 output, unbatched problems. */
  void* sign_out;
  /* flag 32, the reference-precision ("bf16x3") mode: every activation is a PAIR of bf16 planes, value = hi + lo with
   * hi = bf16(v), lo = bf16(v - hi) (16 significand bits), every weight likewise; the caller lists the three products
   * x_hi.w_hi + x_hi.w_lo + x_lo.w_hi as 3x the taps (tap_src_off selects the operand plane, the weight row is the
   * concatenation [w_hi | w_lo | w_hi]) so they accumulate in the same fp32 registers.  dst / res then name the hi plane and
   * the lo plane sits dst_pair_off / res_pair_off ELEMENTS behind it (multiples of 8); `mask` must be a 1-bit tensor;
   * with flag 2 the output is plain fp32 and no residual / mask is applied.  Reference arithmetic: fp32 everywhere
   * (adv/attack.py:20-23, autopgd_base.py:271-289); this mode reproduces it to ~1e-5 of the logit scale. */
  int64_t dst_pair_off, res_pair_off;
  /* train-mode forward (nullable): per 128-row tile of the output, the column sums and sums of squares of the bf16 values as stored,
   * fp32 [ceil(rows / 128)][2][n_cols] -- the batch statistics of the BatchNorm that follows (rart_bn_train_forward_bf16's
   * stats_partial), from the accumulators instead of a pass over the tensor.  Plain bf16 convolution only: no bias / residual / mask /
   * flags, unbatched. */
  float* bn_stats_out;
} rart_conv_desc;

int rart_conv_igemm_bf16(const rart_conv_desc* desc_host, rart_stream_t stream);
/* Tuning knob: problems with n_taps*k_per_tap >= k (and k_per_tap % 64 == 0) use the 128x{128,64}x64 pipeline
 * (default 1024); others the x32 pipeline with loads two K steps ahead. */
int rart_igemm_set_bk64_min_k(long long k);
/* Tuning knob: plain row-major products (one tap, unit strides, no batching, flags within GELU / GELU') with at least 512 tiles of
 * 256 x 256 run on the 8-wave 256 x 256 x 64 kernel with direct-to-LDS tiles (the transformer layers): 2 (default) = on the ping-pong
 * schedule of round 6 (k_gemm256_pp: the two halves of the workgroup alternate memory and matrix phases, counted vmcnt, vector-free
 * buffer_load ... lds issue), 1 = on round 2's two-stage loop (bit-identical outputs), 0 disables the kernel. */
/* Small-M product C[m][n] = A[m][k] . W[n][k]^T (+ bias[n]) for the classifier head and its backward (m = the batch): one workgroup per
 * 32 x 32 output tile, four waves split k (k % 64 == 0), fragments straight from global memory.  out: fp32 (out_is_f32) or bf16, leading
 * dimension ldo.  Replaces the 16-workgroup implicit-GEMM launch of the fc layer (RobustART/model -> public ResNet-50 `fc`). */
int rart_gemm_small_m_bf16(const void* a, int lda, const void* w, int ldw, const float* bias, void* out, int ldo, int out_is_f32, int m,
                           int n, int k, rart_stream_t stream);
int rart_igemm_set_gemm256(int enable);
/* 1 when a plain product of `rows` x k (leading dimension src_ld) by n_cols columns takes the 256 x 256 GEMM kernel -- the only kernel that
 * serves flag 64 (GELU with the pre-activation kept: dst = gelu(u), `mask` RECEIVES the bf16 pre-activation u; ViT fc1 in keep mode). */
int rart_gemm256_supported(long long rows, int k, int n_cols, int src_ld, int dst_ld);

/* Split-bf16 ("fp32x" / "bf16x3") GEMM -- the dense contraction of the REFERENCE-PRECISION engines (csrc/gemm_pair.hip).  The
 * reference computes fp32 (adv/attack.py:20-23, autopgd_base.py:271-289; exprs/exp/imagenet_c_loop_mini/config_vit_base.yaml:1-9 has
 * no precision key).  Every operand is a PAIR of bf16 planes, value = hi + lo (16 significand bits):
 *     C[m][n] = sum_k A[m][k] * W[n][k] ~= A_lo.W_hi + A_hi.W_lo + A_hi.W_hi        (fp32 accumulation, + bias[n])
 * 256 x 256 tiles, the four operand planes of a 32-deep K step staged once in LDS (direct-to-LDS loads), three MFMAs per fragment pair.
 * a_* : [rows][lda] bf16, K contiguous; w_* : [w_rows][ldw] bf16 (rows = output columns; rows >= w_rows read as zeros, so N may exceed
 *       the rows that exist: attention products whose "weights" are activations); K % 32 == 0, N % 8 == 0, ld* % 8 == 0.
 * dst : pair planes [rows][ldc] (hi = bf16(v), lo = bf16(v - hi)), or fp32 [rows][ldc] in dst_hi with flag 2 (dst_lo unused).
 * res : optional residual PAIR indexed like dst, added in fp32.
 * 256- or 128-row tiles x 64 / 128 / 256-column tiles (chosen from the shape; tile_m / tile_n override).
 * flags: 1 ReLU; 2 fp32 output; 4 exact GELU (of the value the pair of the pre-activation represents, as flag 64 computes it); 64 GELU with the pre-activation kept (aux RECEIVES the pair u, dst = gelu(u_hi + u_lo));
 *        8 GELU' (v *= gelu'(aux_hi + aux_lo), aux indexed like dst); the three GELU forms are served by plain products only (conv mode
 *        refuses them with RART_ERR_INVALID);
 *        16 (round 5) the weight table is INTERLEAVED: a row holds, per 32-deep K step, the 32 hi elements followed by the 32 lo elements
 *        (ldw >= 2 K, w_lo = w_hi + 32 elements): one 128-byte line per row and step instead of two half lines K apart.
 * Row re-basing (0 = none): output row m of image m / rows_per_image reads source row img * src_rows_per_image + m % rows_per_image +
 * src_row_off and writes destination row img * dst_rows_per_image + m % rows_per_image + dst_row_off (ViT's class-token slot).
 * Batched (n_batched > 1, blockIdx.y = z -> zo = z / z_inner, zi = z % z_inner): element offsets zo * *_z_outer + zi * *_z_inner are
 * added to a_* / w_* / (dst, res, aux).  rart_gemm_pair_plan_bf16 (below) describes the launches this entry makes for a descriptor. */
typedef struct rart_gemm_pair_desc {
  const void *a_hi, *a_lo, *w_hi, *w_lo;
  const float* bias;
  const void *res_hi, *res_lo;
  void *dst_hi, *dst_lo;
  void *aux_hi, *aux_lo;
  int M, N, K, lda, ldw, ldc, w_rows;
  int rows_per_image, src_rows_per_image, src_row_off, dst_rows_per_image, dst_row_off;
  int flags, n_batched, z_inner;
  int64_t a_z_outer, a_z_inner, w_z_outer, w_z_inner, c_z_outer, c_z_inner;
  /* conv = 1: implicit-GEMM convolution, the row / tap / destination conventions of rart_conv_desc: row m = (image, oy, ox) of a
   * batch x grid_h x grid_w grid, k = tap * k_per_tap + c (k_per_tap a power of two >= 32, <= 16 taps), source pixel
   * (oy sy + tap_dy, ox sx + tap_dx) of a src_h x src_w image with lda elements per pixel (zeros outside), destination pixel
   * (oy dst_sy + dst_oy, ox dst_sx + dst_ox) of a dst_h x dst_w image with ldc elements per pixel; M and K are derived.
   * mask_bits: 1-bit tensor indexed like dst (byte (off + col) / 8, bit col % 8), the value is zeroed where the bit is clear (the
   * ReLU mask of a backward-to-input); sign_out receives (output hi plane > 0) in the same indexing.  Unbatched, no row re-basing. */
  int conv, batch, grid_h, grid_w, src_h, src_w, sy, sx, k_per_tap, n_taps;
  int tap_dy[16], tap_dx[16];
  int dst_h, dst_w, dst_sy, dst_sx, dst_oy, dst_ox;
  const void* mask_bits;
  void* sign_out;
  int tile_n;               /* 0 = automatic (64 / 128 / 256 by N); tests / sweeps force a column tile */
  int tile_m;               /* 0 = automatic (256; 128 for short-K or small convolutions; 224 where it saves a pass); 128 / 224 / 256 force it */
} rart_gemm_pair_desc;
int rart_gemm_pair_bf16(const rart_gemm_pair_desc* desc_host, rart_stream_t stream);
/* The same launch with a SECOND A source whose product lands in the same accumulation (a projection shortcut folded into the 1x1 it is
 * added to): yc = relu(W3 . yb + Wds . x_strided + (b3 + bds)) without the shortcut's tensor ever reaching memory.  `one` describes the
 * launch as rart_gemm_pair_bf16 takes it, conv = 1 (unbatched, no row re-basing).  The second source has one tap at offset 0: row
 * m = (image, oy, ox) reads pixel (oy sy2, ox sx2) of a src2_h x src2_w image with lda2 elements per pixel, k2 channels (a multiple of 32;
 * every row's pixel inside the image).  K of the launch = k_per_tap * n_taps + k2: the K steps of the first source run first, then those
 * of the second, and the weight table's rows are [W1 | W2] along K (one.ldw covers both).  a2_hi null: exactly rart_gemm_pair_bf16(&one).
 * Served under schedules 0 and 1 (224-row tiles included); under the opt-in schedules 2 and 3 such a launch takes the ping-pong kernel.
 * A descriptor of its own, so that every caller of rart_gemm_pair_bf16 keeps its layout.  rart_gemm_pair_max_sources: how many A sources
 * the loaded library takes per launch (2); the engines fold a shortcut only where it says so.  rart_gemm_pair_plan_bf16 describes its launches. */
typedef struct rart_gemm_pair2_desc {
  rart_gemm_pair_desc one;
  const void *a2_hi, *a2_lo;
  int lda2, k2, src2_h, src2_w, sy2, sx2;
} rart_gemm_pair2_desc;
int rart_gemm_pair2_bf16(const rart_gemm_pair2_desc* desc_host, rart_stream_t stream);
int rart_gemm_pair_max_sources(void);
/* Up to four CLASSES of one conv-mode pair launch in ONE grid (blockIdx.y = class): the input-parity classes of a stride-2 backward-to-input,
 * which otherwise run as one launch each, every one quantised into passes over the CUs on its own.  `two.one` describes what the classes
 * share: the row grid, N, the source and destination geometry and strides, k_per_tap, the planes, the mask, the flags; its tap_dy / tap_dx
 * hold the taps of ALL classes (n_taps = how many of the sixteen slots are filled) and its dst_oy / dst_ox are not read.  A class is
 *   taps tap_begin .. tap_begin + n_taps - 1 of those slots,
 *   the columns k_off .. k_off + K - 1 of the rows of the weight table (K = k_per_tap * n_taps, + two.k2 with src2; k_off % 8 == 0): the
 *     per-class tables laid out side by side in one table whose hi and lo planes are w_hi and w_lo, rows ldw apart,
 *   the destination origin (dst_oy, dst_ox),
 *   src2 = 1: the class also accumulates the second source `two` describes (its K steps after the class's own).  Class 0 only.
 * Every output element is the sum of the same products in the same order as in the class's own rart_gemm_pair_bf16 / rart_gemm_pair2_bf16
 * launch: the same bits.  The grid is ordered longest K first.  Tile policy is per launch: the tiles the longest class would choose serve
 * all of them (measured faster than one launch per tile form).  No interleaved weight table (flag 16), no batching, no row re-basing.
 * rart_gemm_pair_max_classes: how many classes the loaded library takes per launch (4); the engines use the entry only where it says so.
 * rart_gemm_pair_plan_bf16 describes its launches. */
typedef struct rart_gemm_pair_class {
  int tap_begin, n_taps, k_off, dst_oy, dst_ox, src2;
} rart_gemm_pair_class;
typedef struct rart_gemm_pair_cls_desc {
  rart_gemm_pair2_desc two;
  int n_classes, reserved_;
  rart_gemm_pair_class cls[4];
} rart_gemm_pair_cls_desc;
int rart_gemm_pair_classes_bf16(const rart_gemm_pair_cls_desc* desc_host, rart_stream_t stream);
int rart_gemm_pair_max_classes(void);
/* Schedule of the 256-row tiles with 128 / 256 columns (round 6, csrc/gemm_pair_pp.hip): 1 (default; RART_PAIR_SCHEDULE in the environment
 * sets the initial value) = ping-pong -- the two halves of the workgroup alternate memory and matrix phases, counted vmcnt, no drain in the
 * steady state; 2 (opt-in: measured slower than 1, see the kernel's header) = ping-pong, and one-tap problems (1x1 convolutions, plain
 * products without row re-basing / batching / GELU) with at least two 256 x 128 tiles per CU on the PERSISTENT kernel, which writes a tile
 * out under the next tile's K loop; 3 (opt-in: measured equal to 1) = ping-pong, and launches of more than one tile per CU WALKED by one
 * workgroup per CU (the next tile's first stage requested before the epilogue); 0 = the two-stage loop of round 4 everywhere.  Under 1 - 3 a
 * plain product whose 256 x 256 tiles fill every XCD's CUs a whole number of times and then less than half of them once more is issued as
 * two launches, the remaining rows on 256 x 128 tiles (RART_PAIR_SPLIT=0 in the environment disables it), and a launch whose row tiles
 * fill an XCD's 32 CUs badly runs tiles that step 224 rows (RART_PAIR_ROWS224=0 disables it).  Outputs are bit-identical under
 * all of these (same products, same order, same point-wise code). */
int rart_gemm_pair_set_schedule(int mode);
int rart_gemm_pair_get_schedule(void);
/* What rart_gemm_pair_bf16 / rart_gemm_pair2_bf16 / rart_gemm_pair_classes_bf16 would launch for a descriptor, without touching the device:
 * the descriptor is checked as those entries check it (same status, same error string), then planned under the current schedule and lab
 * variables for a device of `cus` compute units (<= 0: the current device's, 256 where there is none).  n_classes == 0: no class table
 * (two.a2_hi null: one source).  No operand is read.  A plan is one launch, or two for the remainder split: launch[1] starts where
 * launch[0] ends.  A launch covers rows m_begin .. M - 1 in tiles of tile_m x tile_n that step tile_rows rows (tile_m, or tile_m - 32:
 * the tile's last 32-row block is left out); grid_x x grid_y workgroups of `block` threads.  walk_wgs > 0: the grid_x = min(walk_wgs,
 * tiles) workgroups walk the tiles (ping-pong, schedule 3) or each a run of them (persistent, schedule 2), grid_y == 1. */
enum { RART_GP_TWO_STAGE = 0 /* k_gemm_pair */, RART_GP_PING_PONG = 1 /* k_gemm_pair_pp */, RART_GP_PERSISTENT = 2 /* k_gemm_pair_ps */ };
typedef struct rart_gemm_pair_launch_rec {
  int family, tile_m, tile_n, tile_rows, m_begin, M;
  unsigned grid_x, grid_y, walk_wgs, block;
} rart_gemm_pair_launch_rec;
typedef struct rart_gemm_pair_plan {
  int n_launches, reserved_;
  rart_gemm_pair_launch_rec launch[2];
} rart_gemm_pair_plan;
int rart_gemm_pair_plan_bf16(const rart_gemm_pair_cls_desc* desc_host, int cus, rart_gemm_pair_plan* out);

/* The short-K wide 1x1 pair products of ResNet-50's identity blocks with the A rows resident in registers (csrc/expand_walk_pair.hip): a
 * workgroup owns tile_rows rows (128 or 64; 0 = the library's default) and walks the N columns in chunks of 64 -- all of them, or with
 * col_parts = 2 / 4 (0 = the library's default; a divisor of N / 64) a half / a quarter -- so the A planes go through the load path
 * col_parts times instead of N / 64 times.  The descriptor is rart_gemm_pair_bf16's, restricted to what those launches use: conv = 1, one
 * tap at (0, 0), stride 1, source = row grid = destination pixels (dst_s* = 1, dst_o* = 0), K = k_per_tap = 128 or 256, N a multiple of
 * 64, ldc = N, a pair destination; bias, residual pair, mask_bits, sign_out and the ReLU flag as there (no other flag, no aux, no batching,
 * no row re-basing; tile_m / tile_n are ignored).  Same products in the same order per output element and the same point-wise tail: every
 * output bit equals rart_gemm_pair_bf16's.  rart_expand_walk_pair_max_k: the longest K the loaded library takes (256); the engine uses
 * the entry only where it says so. */
int rart_expand_walk_pair(const rart_gemm_pair_desc* desc_host, int tile_rows, int col_parts, rart_stream_t stream);
int rart_expand_walk_pair_max_k(void);

/* The second half of a ResNet Bottleneck of the reference-precision engine as ONE launch (csrc/conv_tail_pair.hip): 3x3 stride-1 pad-1
 * convolution (c_mid -> c_mid channels, c_mid = 64 or 128) + point-wise step + the 1x1 expansion (c_mid -> 4 c_mid) + skip pair +
 * point-wise step, on hi + lo planes of bf16 with three MFMA products per contraction; the c_mid-channel intermediate stays in registers.
 *   forward  (Bottleneck.forward, conv2-bn2-relu-conv3-bn3-add-relu):  relu_mid = relu_out = 1, biases set, sign_* receive the 1-bit
 *            (value > 0) tensors the backward masks with;
 *   backward (autograd of attack.py:21-22 / autopgd_base.py:271-289 through conv1^T after conv2^T): tables transposed / taps flipped,
 *            mask_mid / mask_out = those 1-bit tensors, res = the gradient arriving over the identity skip.
 * w_*: the 3x3's table, row = output channel, k = tap * c_mid + c, row stride ldw elements.  t_*: the 1x1's [4 c_mid][c_mid] matrix
 * in MFMA fragment order: element ((blk * (c_mid / 16) + s) * 64 + h * 32 + r) * 8 + e = T[blk * 32 + r][16 s + 8 h + e].
 * 1-bit tensors: byte (position * channels + channel) / 8, bit channel % 8. */
typedef struct rart_conv_tail_desc {
  const void* a_hi;  const void* a_lo;       /* input pair [batch][h][w][c_mid] */
  const void* w_hi;  const void* w_lo;
  const void* t_hi;  const void* t_lo;
  const float* bias_mid;                     /* [c_mid] or null */
  const float* bias_out;                     /* [4 c_mid] or null */
  const void* mask_mid;  const void* mask_out;
  void* sign_mid;  void* sign_out;
  const void* res_hi;  const void* res_lo;   /* skip pair [batch][h][w][4 c_mid] or null */
  void* dst_hi;  void* dst_lo;               /* [batch][h][w][4 c_mid] */
  int batch, h, w, c_mid, ldw, relu_mid, relu_out;
  int tap_dy[9], tap_dx[9];                  /* source pixel of tap i = (y + tap_dy[i], x + tap_dx[i]); zero outside the image */
  /* optional (n_hi != null): the NEIGHBOURING block's 1x1 reduction (4 c_mid -> c_mid) of the tile just produced -- forward: the next
   * block's conv1 + bias + ReLU (+ sign tensor); backward: the previous block's conv3^T + mask.  n_*: its [c_mid][4 c_mid] matrix in
   * fragment order by 64-wide K chunk: element (((chunk * (c_mid / 32) + blk) * 4 + s) * 64 + h * 32 + r) * 8 + e =
   * N[blk * 32 + r][64 chunk + 16 s + 8 h + e].  dstn_*: [batch][h][w][c_mid]. */
  const void* n_hi;  const void* n_lo;
  const float* bias_next;
  const void* mask_next;
  void* sign_next;
  void* dstn_hi;  void* dstn_lo;
  int relu_next;
  /* optional (x_hi != null; c_mid = 64, res null): the block's stride-1 1x1 PROJECTION SHORTCUT as extra K steps of the 1x1 -- x_*: its
   * input pair [batch][h][w][64]; tx_*: its [4 c_mid][64] matrix in the fragment order of t_*; bias_out then holds the sum of both biases:
   * dst = relu(T . mid + TX . x + bias_out). */
  const void* x_hi;  const void* x_lo;
  const void* tx_hi;  const void* tx_lo;
} rart_conv_tail_desc;
int rart_conv3x3_tail_pair_supported(int c_mid);
int rart_conv3x3_tail_pair(const rart_conv_tail_desc* desc_host, rart_stream_t stream);
/* How rart_conv3x3_tail_pair brings the 3x3's input to LDS.  1 (default): launches with c_mid = 64, w <= 59 and taps within the 3 x 3
 * neighbourhood stage the positions a 128-position tile reads over all nine taps ONCE per tile (a slab of 128 + 2 (w + 1) rows) and mask
 * out-of-image taps per lane; 0: every launch stages 128 rows per tap, as the c_mid = 128 launches always do.  Outputs are bit-identical
 * (same products, same order).  RART_TAIL_STAGING in the environment sets the initial value. */
int rart_conv3x3_tail_pair_set_staging(int mode);
int rart_conv3x3_tail_pair_get_staging(void);
/* How the launches that take the slab path above read the fragment table of the 1x1 expansion.  1 (default): each 64-output-channel
 * chunk of the table reaches LDS once per workgroup (LDS DMA into the bytes the slab leaves free, two buffers) and all four waves read
 * their fragments from there; 0: every wave loads every fragment from L2 itself.  The tables of the neighbour's reduction and of the
 * shortcut always come from L2; launches off the slab path always use direct loads.  Outputs are bit-identical (same products, same
 * order).  RART_TAIL_TABLES in the environment sets the initial value. */
int rart_conv3x3_tail_pair_set_tables(int mode);
int rart_conv3x3_tail_pair_get_tables(void);

/* Row / elementwise kernels of the reference-precision ViT-B/16 engine (soft-max rows: csrc/vit_pair.hip; unpatchify: csrc/vit_bwd.hip, one kernel for bf16 and fp32 patches; layernorm
 * and its backward: csrc/row_norm.hip, one kernel per direction for this storage and for bf16; add_pos_cls: csrc/vit_aux.hip,
 * likewise): every tensor a pair of bf16 planes, the arithmetic in fp32 as the fp32 module (timm ViT-B/16,
 * RobustART/model/__init__.py:1 -> absent submodule) does it.
 * add_pos_cls: x[b][0][:] = cls_pos0, x[b][t][:] += pos[t].  layernorm: eps inside the root, biased variance; rows of dim <= 1024.
 * layernorm_bwd: dx = rstd (g - mean(g) - xhat mean(g xhat)) [+ res pair], g = dy gamma.  softmax_rows: P = softmax(scale S) of fp32
 * scores (the pair GEMM's fp32 output), zero beyond n_valid up to ld_out (<= 256 columns).  softmax_bwd_rows: dS = scale P (dP - <P, dP>),
 * dP fp32.  unpatchify_from_f32: fp32 patch gradients -> fp32 NCHW image gradient / std. */
int rart_vit_add_pos_cls_pair(void* x_hi, void* x_lo, const float* cls_pos0, const float* pos, int n, int tokens, int dim,
                              rart_stream_t stream);
int rart_layernorm_pair(const void* x_hi, const void* x_lo, const float* gamma, const float* beta, void* out_hi, void* out_lo, int rows,
                        int dim, int64_t in_row_stride, int64_t out_row_stride, float eps, rart_stream_t stream);
int rart_layernorm_bwd_pair(const void* dy_hi, const void* dy_lo, const void* x_hi, const void* x_lo, const float* gamma,
                            const void* res_hi, const void* res_lo, void* dx_hi, void* dx_lo, int rows, int dim, int64_t dy_row_stride,
                            int64_t x_row_stride, int64_t res_row_stride, int64_t dx_row_stride, float eps, rart_stream_t stream);
int rart_softmax_rows_pair(const float* scores, void* probs_hi, void* probs_lo, int64_t rows, int n_valid, int ld_in, int ld_out,
                           float scale, rart_stream_t stream);
int rart_softmax_bwd_rows_pair(const void* probs_hi, const void* probs_lo, const float* dprobs, void* ds_hi, void* ds_lo, int64_t rows,
                               int n_valid, int ld_p, int ld_dp, int ld_out, float scale, rart_stream_t stream);
int rart_vit_unpatchify_from_f32(const float* dpatches, float* grad, int n, int h, int w, int patch, int64_t ld, const float* std_host,
                                 rart_stream_t stream);
/* Fused multi-head self-attention on pairs (head_dim 64), the RESIDENT form: 1 <= tokens <= 224, one workgroup per (image, head) with the
 * item's K and V in LDS (more tokens are refused: rart_vit_attention_stream_pair has no such limit).  qkv pair [n*tokens][3*D]
 * (q | k | v column blocks, heads of 64 inside each) -> out pair [n*tokens][D] = softmax(q k^T / 8) v, every contraction three MFMA
 * products, the soft-max in fp32 registers (timm Attention.forward; the reference runs it in fp32).  The planes have no slack rows. */
int rart_vit_attention_pair(const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, int n, int tokens, int heads, int head_dim,
                            rart_stream_t stream);
/* Its backward (two launches, csrc/vit_pair.hip; head_dim 64, 1 <= tokens <= 224): dqkv pair [n*tokens][3*D] (dq | dk | dv) from the qkv
 * pair, the forward's output pair, and the gradient pair of that output.  stats: scratch of n * heads * 32 * ceil(tokens / 32) * 4 floats
 * (per query: max, 1 / sum, delta). */
int rart_vit_attention_bwd_pair(const void* qkv_hi, const void* qkv_lo, const void* out_hi, const void* out_lo, const void* dout_hi,
                                const void* dout_lo, void* dqkv_hi, void* dqkv_lo, float* stats, int n, int tokens, int heads, int head_dim,
                                rart_stream_t stream);
/* The same attention and its backward, STREAMING (csrc/vit_stream.hip): head_dim 64, any tokens >= 1 (up to 2^20; a shape beyond the
 * kernels' 32-bit indices is refused with a message).  One workgroup per (image, head, block of at most eight 32-query tiles); K / V
 * (backward, key side: Q / dO and the statistics) pass through LDS in chunks of 64 rows, the forward keeps a running maximum and sum per
 * query.  Layouts, the three products per contraction and the stats formula are those of the resident entries; rows past n*tokens of
 * any plane are never read.  No atomics: results are bit-reproducible and an image's rows do not depend on the batch. */
int rart_vit_attention_stream_pair(const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, int n, int tokens, int heads,
                                   int head_dim, rart_stream_t stream);
int rart_vit_attention_bwd_stream_pair(const void* qkv_hi, const void* qkv_lo, const void* out_hi, const void* out_lo, const void* dout_hi,
                                       const void* dout_lo, void* dqkv_hi, void* dqkv_lo, float* stats, int n, int tokens, int heads,
                                       int head_dim, rart_stream_t stream);

/* 3x3 stride-1 "same" convolution, channels in = channels out = 64, 128 or 256 (256: images of at most 224 positions, one
 * image per workgroup), bf16 NHWC, with the input halo tile resident in LDS (csrc/conv3x3_halo.hip): ResNet-50's layer1 /
 * layer2 / layer3 conv2, forward (taps (r-1, s-1), bias + ReLU, sign_out =
 * 1-bit mask of the output) and backward-to-input (taps (1-r, 1-s), weights [cin][tap*cout+co], mask_bits = 1-bit ReLU
 * mask of the destination).  wgt: the bf16 table [channels][9*channels] (k = tap*channels + c) RE-ORDERED by
 * rart_conv3x3_pack_frag_bf16 into MFMA-fragment order (fragment (K step st of 64, column tile wn, ks) = 64 lanes x 8
 * elements, lane l = w[wn*32 + (l & 31)][st*64 + ks*16 + (l >> 5)*8 ..]: a fragment load reads 1 KiB contiguous).  Any pointer
 * of bias / mask_bits / sign_out may be NULL.  rart_conv3x3_halo_supported: 1 when the geometry fits the LDS tile
 * (otherwise use rart_conv_igemm_bf16, which computes the same function). */
int rart_conv3x3_halo_supported(int channels, int h, int w);
int rart_conv3x3_pack_frag_bf16(const void* w_rows, void* w_frag, int channels, rart_stream_t stream);
/* The same re-ordering for any bf16 [rows][k] row-major matrix (rows % 32 == 0, k % 64 == 0): fragment (st, wn, ks) as above. */
int rart_pack_frag_bf16(const void* w_rows, void* w_frag, int rows, int k, rart_stream_t stream);
int rart_conv3x3_halo_bf16(const void* src, const void* wgt, const float* bias, const void* mask_bits, void* sign_out,
                           void* dst, int n, int h, int w, int channels, const int* tap_dy, const int* tap_dx, int relu,
                           rart_stream_t stream);

/* Grouped 3x3 convolution, channels in = channels out, groups of group_width = 4, 8, 16, 32 or 64 channels, NHWC, bf16 or split-bf16
 * (hi + lo planes, the three products hi.hi + hi.lo + lo.hi as rart_gemm_pair_bf16 forms them) with the source tile of a workgroup
 * resident in LDS (csrc/conv_grouped.hip): conv2 of a ResNeXt Bottleneck, forward and backward-to-input.  The channels are cut into
 * slices of S = 32 consecutive channels (64 when group_width is 64); a slice holds whole groups and reads only itself.
 *   dst(b, y * dst_stride + dst_oy, x * dst_stride + dst_ox, :) = act(sum_t W_t . src(b, y * stride + tap_dy[t], x * stride + tap_dx[t], :)
 *   + bias) for the pixels (y, x) of a grid_h x grid_w grid; source pixels outside src_h x src_w read zero.  1 <= n_taps <= 9, taps in
 * -1 .. 1, stride 1 or 2, the grid must map inside dst_h x dst_w.  One entry serves the forward (stride 1 / 2, dst_stride 1), the backward
 * at stride 1 (flipped taps, per-group transposed weights) and each input-parity class of the stride-2 backward (stride 1, dst_stride 2,
 * origin = the parity, the 1 / 2 / 2 / 4 taps of the class).
 * wgt: per slice s the dense bf16 table T_s [S out][n_taps * S in] (k = tap * S + c, exact zeros off the block diagonal of the groups)
 * in MFMA-fragment order: element (((s * n_taps * S / 16 + st) * (S / 32) + j) * 64 + l) * 8 + e = T_s[j * 32 + (l & 31)][st * 16 +
 * (l >> 5) * 8 + e].  bias fp32 [channels]; mask_bits: 1 bit per destination element (byte e / 8 of element offset e), the value is zeroed
 * where clear; sign_out: receives (stored hi value > 0), same indexing; relu: applied last.  bias / mask_bits / sign_out may be NULL.
 * dst must not alias src.  rart_conv3x3_grouped_supported(channels, group_width, h, w, stride): 1 when the entries take a source of
 * h x w pixels at this stride; where it says 0 they return RART_ERR_INVALID and write nothing.  rart_conv3x3_grouped_tile: the output
 * pixels (rows x cols) one workgroup owns for this slice width, storage (pair != 0: split-bf16) and stride. */
int rart_conv3x3_grouped_supported(int channels, int group_width, int h, int w, int stride);
int rart_conv3x3_grouped_tile(int group_width, int pair, int stride, int* rows, int* cols);
int rart_conv3x3_grouped_bf16(const void* src, const void* wgt, const float* bias, const void* mask_bits, void* sign_out, void* dst, int n,
                              int src_h, int src_w, int channels, int group_width, int stride, int grid_h, int grid_w, int n_taps,
                              const int* tap_dy, const int* tap_dx, int dst_h, int dst_w, int dst_stride, int dst_oy, int dst_ox, int relu,
                              rart_stream_t stream);
int rart_conv3x3_grouped_pair(const void* src_hi, const void* src_lo, const void* wgt_hi, const void* wgt_lo, const float* bias,
                              const void* mask_bits, void* sign_out, void* dst_hi, void* dst_lo, int n, int src_h, int src_w, int channels,
                              int group_width, int stride, int grid_h, int grid_w, int n_taps, const int* tap_dy, const int* tap_dx,
                              int dst_h, int dst_w, int dst_stride, int dst_oy, int dst_ox, int relu, rart_stream_t stream);

/* DenseNet's element kernels (csrc/densenet.hip), NHWC rows, bf16 or split-bf16 (hi + lo planes; the *_pair entries).  c = the channel
 * count C, a positive multiple of 32; every row stride ld >= C with ld % 8 == 0; rows (or n * h * w) in 1 .. 2^31 - 1; tensors 16-byte
 * aligned, sign tensors 4-byte; s, t: fp32 [C], the folded BatchNorm (scale, shift).  Anything else is RART_ERR_INVALID before any launch.
 * The arithmetic is fp32 on hi + lo: a = fma(s, x, t), ReLU (a NaN stays a NaN), then one round-to-nearest-even into the storage.
 *   rart_dn_preact_*: y[r][c] = relu(s[c] x[r][c] + t[c]) for c < C.  x: rows of stride ld_x (a channel prefix of a wider buffer, read
 *     only); y: dense [rows][C].  sign_out (or NULL): 1 bit per element of y, byte (r * C + c) / 8, bit c & 7, set exactly when the
 *     stored (hi) value is > 0.
 *   rart_dn_preact_bwd_*: g[r][c] (accumulate = 0: =, 1: +=) bit[r][c] * s[c] * d[r][c] for c < C.  d: dense [rows][C]; bits: the sign
 *     tensor of the forward; g: rows of stride ld_g, channels >= C of a row are neither read nor written; s may be NULL (= 1: the
 *     caller folded it into the table that produced d).
 *   rart_dn_preact_pool2_*: the same pre-activation followed by a 2 x 2 / 2 average pool (a transition: the pool commutes with the
 *     bias-free 1x1 convolution after it).  x: [n][h][w] pixels of stride ld_x, h and w even; y: dense [n][h / 2][w / 2][C], the mean of
 *     the four activated values, rounded once; sign_out (or NULL): [n][h][w][C / 8] at FULL resolution, bit = activated value > 0.
 *   rart_dn_preact_pool2_bwd_*: g[b][y][x][c] (=|+=) bit * s[c] * d[b][y / 2][x / 2][c] / 4.  d: dense [n][h / 2][w / 2][C].
 *   rart_dn_copy_*: dst[r][c] = src[r][c] for c < C, rows of stride ld_src / ld_dst: a channel slice into or out of a concat buffer. */
int rart_dn_preact_bf16(const void* x, int ld_x, const float* s, const float* t, void* y, void* sign_out, long long rows, int c,
                        rart_stream_t stream);
int rart_dn_preact_pair(const void* x_hi, const void* x_lo, int ld_x, const float* s, const float* t, void* y_hi, void* y_lo, void* sign_out,
                        long long rows, int c, rart_stream_t stream);
int rart_dn_preact_bwd_bf16(const void* d, const void* bits, const float* s, void* g, int ld_g, int accumulate, long long rows, int c,
                            rart_stream_t stream);
int rart_dn_preact_bwd_pair(const void* d_hi, const void* d_lo, const void* bits, const float* s, void* g_hi, void* g_lo, int ld_g, int accumulate,
                            long long rows, int c, rart_stream_t stream);
int rart_dn_preact_pool2_bf16(const void* x, int ld_x, const float* s, const float* t, void* y, void* sign_out, int n, int h, int w, int c,
                              rart_stream_t stream);
int rart_dn_preact_pool2_pair(const void* x_hi, const void* x_lo, int ld_x, const float* s, const float* t, void* y_hi, void* y_lo,
                              void* sign_out, int n, int h, int w, int c, rart_stream_t stream);
int rart_dn_preact_pool2_bwd_bf16(const void* d, const void* bits, const float* s, void* g, int ld_g, int accumulate, int n, int h, int w,
                                  int c, rart_stream_t stream);
int rart_dn_preact_pool2_bwd_pair(const void* d_hi, const void* d_lo, const void* bits, const float* s, void* g_hi, void* g_lo, int ld_g,
                                  int accumulate, int n, int h, int w, int c, rart_stream_t stream);
int rart_dn_copy_bf16(const void* src, int ld_src, void* dst, int ld_dst, long long rows, int c, rart_stream_t stream);
int rart_dn_copy_pair(const void* src_hi, const void* src_lo, int ld_src, void* dst_hi, void* dst_lo, int ld_dst, long long rows, int c,
                      rart_stream_t stream);

/* One identity BasicBlock of ResNet-18 / -34 (3x3 C -> C, 3x3 C -> C, + the block input; stride 1, "same" padding) as ONE kernel with
 * the intermediate kept on chip (csrc/basic_block.hip); channels 64 or 128, any h, w >= 1 with n * h * w * channels < 2^31.  Replaces the
 * two rart_conv3x3_halo_bf16 / rart_conv_igemm_bf16 launches of the block and does their arithmetic: fp32 accumulation, the intermediate
 * rounded to bf16 once (round-to-nearest-even).  x, out: bf16 NHWC [n][h][w][channels], out != x.  w1, w2: the 3x3 tables
 * [channels][9 * channels] (k = tap * channels + c) in the fragment order of rart_conv3x3_pack_frag_bf16, with ONE tap list for both;
 * b1, b2: fp32 [channels] or NULL.  m_mid / m_io: 1 bit per element of the intermediate / of out, indexed like the activation (byte
 * e / 8, bit e % 8 of element offset e).
 *   backward = 0: out = relu(w2 * relu(w1 * x + b1) + b2 + x); m_mid and m_io are OUTPUTS (stored value > 0), each may be NULL.  A NaN
 *                 stays a NaN through both ReLUs.
 *   backward = 1: x is the gradient at the block output (already masked by that output's ReLU), w1 / w2 the transposed tables of
 *                 conv2 / conv1 with the flipped taps, no biases; out = m_io . (w2 * (m_mid . (w1 * x)) + x) with m_mid = the sign of
 *                 the forward's intermediate (required) and m_io = of the block input (or NULL).
 * Intermediate positions outside the image are zero (the second convolution's padding) and no tile reads a neighbouring image.
 * Tensors must be 16-byte aligned, biases 4-byte.  rart_basic_block_supported: 1 when the entry takes this width and image size; where
 * it says 0 the entry returns RART_ERR_INVALID and writes nothing.  rart_basic_block_tile: the output pixels (rows x cols of one image)
 * a workgroup owns at this width. */
int rart_basic_block_supported(int channels, int h, int w);
int rart_basic_block_tile(int channels, int* rows, int* cols);
int rart_basic_block_bf16(const void* x, const void* w1, const void* w2, const float* b1, const float* b2, void* m_mid, void* m_io,
                          void* out, int n, int h, int w, int channels, const int* tap_dy, const int* tap_dx, int backward,
                          rart_stream_t stream);

/* One identity Bottleneck (1x1 c_io -> c_mid, 3x3 c_mid -> c_mid, 1x1 c_mid -> c_io, + the block input) as ONE kernel with
 * both intermediates kept on chip (csrc/bottleneck_fused.hip); supported geometry: c_io 256, c_mid 64, 56 x 56 (ResNet-50
 * layer1 blocks 1-2).  Replaces three rart_conv_igemm_bf16 / rart_conv3x3_halo_bf16 launches and computes the same function.
 * x, out: bf16 NHWC [n][h][w][c_io], out != x.  w1: bf16 [c_mid][c_io]; w2: the 3x3 table [c_mid][9*c_mid] (k = tap*c_mid + c)
 * re-ordered by rart_conv3x3_pack_frag_bf16 into MFMA-fragment order, with its taps; w3: bf16 [c_io][c_mid]; b1..b3 fp32 or NULL.  m1 / m2 / m3: 1 bit per element of the stage-1 / stage-2 / final
 * result (byte (pos*C + ch) >> 3, bit ch & 7).
 *   backward = 0: out = relu(w3.relu(w2*relu(w1.x + b1) + b2) + b3 + x); m1..m3 are OUTPUTS (value > 0), each may be NULL.
 *   backward = 1: x is the gradient at the block output (already masked by that output's ReLU), w1 / w2 / w3 the transposed
 *                 tables of conv3 / conv2 (flipped taps) / conv1, no biases; out = m3 . (w3.(m2.(w2*(m1.(w1.x)))) + x) with
 *                 m1 = sign of the forward's conv2 output, m2 = of its conv1 output, m3 = of the block input (or NULL). */
int rart_bottleneck_fused_supported(int c_io, int c_mid, int h, int w);
int rart_bottleneck_fused_bf16(const void* x, const void* w1, const void* w2, const void* w3, const float* b1, const float* b2,
                               const float* b3, void* m1, void* m2, void* m3, void* out, int n, int h, int w, int c_io,
                               int c_mid, const int* tap_dy, const int* tap_dx, int backward, rart_stream_t stream);

/* The FIRST Bottleneck of the layer (projection shortcut, stride 1) as one kernel; supported geometry: c_in 64, c_mid 64,
 * c_out 256, 56 x 56 (ResNet-50 layer1 block 0).  Same kernel family and conventions as rart_bottleneck_fused_bf16.
 *   backward = 0: x bf16 [n][h][w][c_in]; w1 [c_mid][c_in]; w2 fragment-ordered 3x3 table; w3 [c_out][c_mid]; w4 = the
 *                 shortcut's [c_out][c_in] table in fragment order (rart_pack_frag_bf16(rows c_out, k c_in)); b3 = conv3 bias +
 *                 shortcut bias; out [n][h][w][c_out] = relu(w3.a2 + w4.x + b3); m1..m3 sign OUTPUTS or NULL.
 *   backward = 1: x = gradient at the block output [n][h][w][c_out]; w1 = conv3's transposed table [c_mid][c_out]; w2 = conv2's
 *                 backward table (fragment order, flipped taps); w3 = the shortcut's transposed table [c_in][c_out]; w4 = conv1's
 *                 transposed table [c_in][c_mid] (row-major); out [n][h][w][c_in] = m3 . (w4.(m2.(w2*(m1.(w1.x)))) + w3.x). */
int rart_bottleneck_first_supported(int c_in, int c_mid, int c_out, int h, int w);
int rart_bottleneck_first_bf16(const void* x, const void* w1, const void* w2, const void* w3, const void* w4, const float* b1,
                               const float* b2, const float* b3, void* m1, void* m2, void* m3, void* out, int n, int h, int w,
                               int c_in, int c_mid, int c_out, const int* tap_dy, const int* tap_dx, int backward,
                               rart_stream_t stream);

/* The FIRST Bottleneck of layer2 / layer3 -- stride 2 on the 3x3, projection shortcut -- FORWARD as one kernel
 * (csrc/bottleneck_s2_fused.hip): out = relu(w3 . relu(w2 *s2 relu(w1 . x + b1) + b2) + wd . x[::2, ::2] + b3), b3 = conv3 bias +
 * shortcut bias.  Supported: c_in 256 -> c_mid 128 -> c_out 512 at 56 x 56 and 512 -> 256 -> 1024 at 28 x 28 (x is h x w, out
 * h/2 x w/2).  All four tables in fragment order: w1 = rart_pack_frag_bf16(rows c_mid, k c_in) of [c_mid][c_in]; w2 = of
 * [c_mid][9*c_mid] with k = (r*3+s)*c_mid + c and taps (r-1, s-1); w3 = of [c_out][c_mid]; wd = of [c_out][c_in].
 * m1 / m2 / m3 (nullable): 1-bit sign OUTPUTS of a1 [n][h][w][c_mid/8], a2 [n][h/2][w/2][c_mid/8], out [n][h/2][w/2][c_out/8].
 * Replaces four rart_conv_igemm_bf16 launches and computes the same function (the shortcut is not rounded to bf16 on its own).
 * Reference: Bottleneck.forward with a downsample branch inside `model(x)` of adv/attack.py:21-22, autopgd_base.py:271-289. */
int rart_bottleneck_s2_fwd_supported(int c_in, int c_mid, int c_out, int h, int w);
int rart_bottleneck_s2_fwd_bf16(const void* x, const void* w1, const void* w2, const void* w3, const void* wd, const float* b1,
                                const float* b2, const float* b3, void* m1, void* m2, void* m3, void* out, int n, int h, int w,
                                int c_in, int c_mid, int c_out, rart_stream_t stream);

/* The backward-to-input of the same stride-2 blocks as one kernel:
 *   dx = m0 . ( w1t . ( m1 . ( w2t *s2^T ( m2 . ( w3t . g ) ) ) ) + wdt . g [at even / even input positions] ),
 * g = bf16 gradient at the block output [n][h/2][w/2][c_out] (already masked by that output's ReLU), dx [n][h][w][c_in].
 * Tables in fragment order (rart_pack_frag_bf16): w3t = conv3's transposed table [c_mid][c_out]; w1t = conv1's [c_in][c_mid];
 * wdt = the shortcut's [c_in][c_out]; w2t = the four input-parity-class tables of the 3x3 / 2's transpose, class order (0,0) (0,1)
 * (1,0) (1,1), class (ph, pw) = [c_mid][ntaps * c_mid] with k = tap * c_mid + c and its taps = the filter taps (r, s) with
 * (ph + 1 - r), (pw + 1 - s) even, r then s ascending (1 / 2 / 2 / 4 taps), each packed on its own and concatenated (element offsets
 * 0, 1, 3, 5 times c_mid^2).  m2 / m1 / m0: the 1-bit sign tensors of a2 / a1 / the block input written by the forward (m0 nullable).
 * Replaces seven rart_conv_igemm_bf16 launches.  Reference: autograd of the same Bottleneck (adv/attack.py:21-22). */
int rart_bottleneck_s2_bwd_bf16(const void* g, const void* w3t, const void* w2t, const void* w1t, const void* wdt, const void* m2,
                                const void* m1, const void* m0, void* dx, int n, int h, int w, int c_in, int c_mid, int c_out,
                                rart_stream_t stream);

/* One identity Bottleneck at 14 x 14 (ResNet-50 layer3 blocks 1-5: c_io 1024, c_mid 256) as one kernel, ONE IMAGE PER WORKGROUP
 * (csrc/bottleneck14_fused.hip).  Same conventions as rart_bottleneck_fused_bf16 (forward / backward, biases, the three 1-bit
 * mask tensors m1 [P][c_mid/8], m2 [P][c_mid/8], m3 [P][c_io/8]), except that ALL THREE weight tables are passed in fragment order:
 * w1 = rart_pack_frag_bf16(rows c_mid, k c_io) of [c_mid][c_io]; w2 = rart_conv3x3_pack_frag_bf16 of [c_mid][9*c_mid];
 * w3 = rart_pack_frag_bf16(rows c_io, k c_mid) of [c_io][c_mid]. */
int rart_bottleneck14_fused_supported(int c_io, int c_mid, int h, int w);
int rart_bottleneck14_fused_bf16(const void* x, const void* w1, const void* w2, const void* w3, const float* b1, const float* b2,
                                 const float* b3, void* m1, void* m2, void* m3, void* out, int n, int h, int w, int c_io,
                                 int c_mid, const int* tap_dy, const int* tap_dx, int backward, rart_stream_t stream);

/* One identity Bottleneck at 28 x 28 (ResNet-50 layer2 blocks 1-3: c_io 512, c_mid 128) as one kernel, a 14 x 14 quarter of an
 * image per workgroup, two workgroups per CU (csrc/bottleneck28_fused.hip).  Conventions and table formats as for
 * rart_bottleneck14_fused_bf16: w1 = rart_pack_frag_bf16(rows c_mid, k c_io), w2 = rart_conv3x3_pack_frag_bf16,
 * w3 = rart_pack_frag_bf16(rows c_io, k c_mid); masks m1 / m2 [P][c_mid/8], m3 [P][c_io/8]. */
int rart_bottleneck28_fused_supported(int c_io, int c_mid, int h, int w);
int rart_bottleneck28_fused_bf16(const void* x, const void* w1, const void* w2, const void* w3, const float* b1, const float* b2,
                                 const float* b3, void* m1, void* m2, void* m3, void* out, int n, int h, int w, int c_io,
                                 int c_mid, const int* tap_dy, const int* tap_dx, int backward, rart_stream_t stream);

/* One identity Bottleneck at 7 x 7 (ResNet-50 layer4 blocks 1-2: c_io 2048, c_mid 512) as one kernel, one image per workgroup
 * (csrc/bottleneck7_fused.hip).  Conventions as for rart_bottleneck14_fused_bf16; all three tables in fragment order:
 * w1 = rart_pack_frag_bf16(rows c_mid, k c_io), w2 = rart_pack_frag_bf16(rows c_mid, k 9*c_mid), w3 = rart_pack_frag_bf16(rows c_io,
 * k c_mid); masks m1 / m2 [P][c_mid/8], m3 [P][c_io/8]. */
int rart_bottleneck7_fused_supported(int c_io, int c_mid, int h, int w);
int rart_bottleneck7_fused_bf16(const void* x, const void* w1, const void* w2, const void* w3, const float* b1, const float* b2,
                                const float* b3, void* m1, void* m2, void* m3, void* out, int n, int h, int w, int c_io,
                                int c_mid, const int* tap_dy, const int* tap_dx, int backward, rart_stream_t stream);

/* src: fp32 NCHW in [0,1] (src_is_u8 = 0) or uint8 NHWC (src_is_u8 = 1) -> (x - mean)/std as two bf16
 * planes hi, lo (hi + lo ~ fp32 value), each [n][h+8][w+8][4] with the image at (3,3) and zeros around:
 * the stem convolution's operand (normalisation of imfgsm_attack.py:14-23 / autoattack.py:17-20 fused). */
int rart_engine_prep_input(const void* src, int src_is_u8, void* hi, void* lo, int n, int h, int w,
                           const float* mean_host, const float* std_host, rart_stream_t stream);
/* 3x3 stride-2 pad-1 max pool on bf16 NHWC; argmax_out (nullable): uint8 [n][h/2][w/2][c], the window
 * position ky*3+kx of the first maximum (PyTorch's rule).  Backward, fused with the ReLU mask of the pool's
 * input y: dz = (y > 0) * sum of dpool over the windows whose argmax is this pixel. */
int rart_engine_maxpool(const void* in, void* out, void* argmax_out, int n, int h, int w, int c,
                        rart_stream_t stream);
/* The same pool, also writing sign_out (nullable): uint8 [n][h/2][w/2][c/8], bit j of byte k = (pooled channel 8k+j > 0)
 * -- the 1-bit ReLU mask the backward GEMMs read with rart_conv_desc flag 16.  argmax code 15 = window maximum <= 0. */
int rart_engine_maxpool_keep(const void* in, void* out, void* argmax_out, void* sign_out, int n, int h, int w, int c,
                             rart_stream_t stream);
int rart_engine_maxpool_bwd(const void* y, const void* argmax, const void* dpool, void* dz, int n, int h, int w,
                            int c, rart_stream_t stream);
/* global average pool [n][hw][c] -> [n][c], and dz = (y > 0) ? dpool / hw : 0. */
int rart_engine_avgpool(const void* in, void* out, int n, int hw, int c, rart_stream_t stream);
int rart_engine_avgpool_bwd(const void* y, const void* dpool, void* dz, int n, int hw, int c, rart_stream_t stream);
/* stem backward: bf16 patches [n][h/2][w/2][patch_cols] (column (r*7+s)*3+c) -> fp32 NCHW gradient w.r.t.
 * the [0,1] image (the 1/std of the normalisation applied). */
int rart_engine_stem_col2im(const void* patches, float* grad, int n, int h, int w, int patch_cols,
                            const float* std_host, rart_stream_t stream);
/* ---- reference-precision ("bf16x3") forms of the pools / converters (csrc/engine_aux.hip) ----------------------------------
 * Every tensor is a PAIR of bf16 planes, value = hi + lo (see rart_conv_desc flag 32): `*_hi` names the hi plane and the lo
 * plane sits `*_lo_off` ELEMENTS behind it (a positive multiple of 8).  Arithmetic: unpack to fp32 (hi + lo is exact),
 * compute as the bf16 kernel of the same name, split again.  Reference: the fp32 max_pool2d / adaptive_avg_pool2d and their
 * autograd inside `model(x)` of adv/attack.py:20-23, autopgd_base.py:271-289. */
int rart_engine_maxpool_pair(const void* in_hi, long long in_lo_off, void* out_hi, long long out_lo_off, void* argmax_out,
                             void* sign_out, int n, int h, int w, int c, rart_stream_t stream);
/* dz (at the pool input, masked by the ReLU in front of the pool) from the argmax codes alone: code 15 marks windows whose
 * maximum is <= 0, any other code names a position whose value is that positive maximum. */
int rart_engine_maxpool_bwd_pair(const void* argmax, const void* dpool_hi, long long dpool_lo_off, void* dz_hi,
                                 long long dz_lo_off, int n, int h, int w, int c, rart_stream_t stream);
int rart_engine_avgpool_pair(const void* in_hi, long long in_lo_off, void* out_hi, long long out_lo_off, int n, int hw, int c,
                             rart_stream_t stream);
/* y_sign_bits: uint8 [n][hw][c/8], the 1-bit (y > 0) tensor the last block's forward GEMM wrote through sign_out. */
int rart_engine_avgpool_bwd_pair(const void* y_sign_bits, const void* dpool_hi, long long dpool_lo_off, void* dz_hi,
                                 long long dz_lo_off, int n, int hw, int c, rart_stream_t stream);
/* fp32 [rows][cols] -> pair [rows][dst_cols] (zero padded): the loss gradient entering the fc backward. */
int rart_f32_to_pair_rows(const float* src, void* dst_hi, long long dst_lo_off, int rows, int cols, int dst_cols,
                          rart_stream_t stream);
/* rart_engine_stem_col2im for fp32 patches (the stem's backward GEMM run with flags 32 | 2); h % 16 == 0, w % 32 == 0. */
int rart_engine_stem_col2im_f32(const float* patches, float* grad, int n, int h, int w, int patch_cols, const float* std_host,
                                rart_stream_t stream);
/* The same stem backward as ONE kernel: pooled gradient dpool [n][h/4][w/4][64] bf16 + the max pool's argmax codes
 * (rart_engine_maxpool; code 15 = window maximum <= 0) -> fp32 NCHW gradient w.r.t. the [0,1] image.  Max-pool backward,
 * the ReLU mask and the transposed 7x7/2 convolution are fused: an implicit GEMM over the 4x4 neighbourhood of
 * stem-output positions (K = 16 taps x 64 channels, N = 4 input parities x 3 channels) on MFMA with the gathered
 * operand built in LDS.  wtab: bf16 [16][1024], row (py*2+px)*3+c, column ((dp+1)*4+(dq+1))*64+k = W[k][c][py+3-2dp][px+3-2dq]
 * (0 where the tap index leaves 0..6; rows 12..15 zero).  h, w multiples of 4.
 * (autograd of attack.py:21-22 / autopgd_base.py:271-289 through conv1-bn1-relu-maxpool) */
int rart_engine_stem_bwd_fused(const void* dpool, const void* argmax, const void* wtab, float* grad, int n, int h, int w,
                               const float* std_host, rart_stream_t stream);
/* The reference-precision stem FORWARD as one persistent kernel (csrc/stem_pair.hip): normalisation + hi / lo split + 7x7/2 convolution
 * (three MFMA products per K step) + bias + ReLU + hi / lo split + 3x3/2 max pool of the pair values; bit-identical to
 * rart_engine_prep_input -> rart_gemm_pair_bf16 (7 row taps) -> rart_engine_maxpool_pair.  wgt_*: [64][224] bf16, column r * 32 + px * 4 + c
 * (px < 7, c < 3; zero elsewhere).  p1_*: [n][h/4][w/4][64]; argmax_out / sign_out as rart_engine_maxpool_pair (may be null). */
int rart_engine_stem_fwd_fused_pair(const void* src, int src_is_u8, const void* wgt_hi, const void* wgt_lo, const float* bias, void* p1_hi,
                                    void* p1_lo, void* argmax_out, void* sign_out, int n, int h, int w, const float* mean_host,
                                    const float* std_host, rart_stream_t stream);
/* The same kernel, which ALSO runs the 1x1 convolution (64 -> 64) + bias + ReLU that reads the pooled pair -- conv1 of layer1's first block
 * -- on each pooled tile before it leaves the CU: that launch's read of the pooled pair disappears.  wnext_*: the table planes [64][ldw_next]
 * bf16 (row = output channel, 64 input channels; ldw_next >= 64, a multiple of 8); next_*: the output pair [n][h/4][w/4][64];
 * next_sign_out: (output hi plane > 0), 1 bit per element (may be null, like bias_next).  Everything else as rart_engine_stem_fwd_fused_pair,
 * with the same p1 / argmax / sign outputs bit for bit; next_* and next_sign_out are bit-identical to rart_gemm_pair_bf16 on p1 (one tap,
 * K = 64, flag 1): the same products in the same order on the same rounded pair. */
int rart_engine_stem_fwd_next_pair(const void* src, int src_is_u8, const void* wgt_hi, const void* wgt_lo, const float* bias, void* p1_hi,
                                   void* p1_lo, void* argmax_out, void* sign_out, const void* wnext_hi, const void* wnext_lo, int ldw_next,
                                   const float* bias_next, void* next_hi, void* next_lo, void* next_sign_out, int n, int h, int w,
                                   const float* mean_host, const float* std_host, rart_stream_t stream);
/* The reference-precision form (csrc/stem_pair.hip): pooled gradient and weight table as hi + lo planes of bf16, three MFMA products per
 * fragment pair; replaces rart_engine_maxpool_bwd_pair -> rart_gemm_pair_bf16 (patches, fp32) -> rart_engine_stem_col2im_f32. */
int rart_engine_stem_bwd_fused_pair(const void* dpool_hi, const void* dpool_lo, const void* argmax, const void* wtab_hi, const void* wtab_lo,
                                    float* grad, int n, int h, int w, const float* std_host, rart_stream_t stream);
/* The stem FORWARD as one persistent kernel: normalisation + hi/lo bf16 split (rart_engine_prep_input), 7x7/2 convolution
 * with the folded BatchNorm bias + ReLU (the K = 448 row-tap GEMM) and the 3x3/2 max pool (rart_engine_maxpool_keep) fused;
 * the 112 x 112 x 64 stem output never reaches HBM.  wgt: bf16 [64][wgt_row_stride], row n, column r*32 + s*4 + c =
 * W[n][c][r][s] (s = 7 and c = 3 zero) -- the hi half of the stem table; outputs as rart_engine_maxpool_keep
 * (p1 bf16 [n][h/4][w/4][64], argmax codes and sign bits nullable).  h, w multiples of 4. */
int rart_engine_stem_fwd_fused(const void* src, int src_is_u8, const void* wgt, int wgt_row_stride, const float* bias,
                               void* p1, void* argmax_out, void* sign_out, int n, int h, int w, const float* mean_host,
                               const float* std_host, rart_stream_t stream);
/* fp32 [rows][cols] -> bf16 [rows][dst_cols] (zero padded): dlogits -> GEMM operand. */
int rart_f32_to_bf16_rows(const float* src, void* dst, int rows, int cols, int dst_cols, rart_stream_t stream);

/* ---- ViT-B/16 forward (model `vit_base`; every matmul incl. attention runs on rart_conv_igemm_bf16) ---- */
/* image -> normalised patches [n][(h/p)*(w/p)][3*p*p] (k = c*p*p + r*p + s, the Conv2d(3, D, p, p) weight order),
 * bf16 hi/lo planes. */
int rart_vit_patchify(const void* src, int src_is_u8, void* hi, void* lo, int n, int h, int w, int patch,
                      const float* mean_host, const float* std_host, rart_stream_t stream);
/* x[b][0] = cls_pos0 (class token + its position embedding); x[b][t] += pos[t] for t >= 1.  x bf16 [n][tokens][dim]. */
int rart_vit_add_pos_cls(void* x, const float* cls_pos0, const float* pos, int n, int tokens, int dim,
                         rart_stream_t stream);
int rart_layernorm_bf16(const void* x, const float* gamma, const float* beta, void* out, int rows, int dim,
                        int64_t in_row_stride, int64_t out_row_stride, float eps, rart_stream_t stream);
/* probs[r][0..n_valid) = softmax(scale * scores[r][0..n_valid)), zeros up to ld_out (the K padding of P.V). */
int rart_softmax_rows_bf16(const void* scores, void* probs, int64_t rows, int n_valid, int ld_in, int ld_out,
                           float scale, rart_stream_t stream);
/* Fused multi-head attention on the fused qkv activation [n][tokens][3*heads*head_dim] (q | k | v, heads contiguous,
 * timm layout): out[n][tokens][heads*head_dim] = softmax(q k^T / sqrt(head_dim)) v, bf16 in/out, fp32 statistics.
 * The RESIDENT form: head_dim == 64, 1 <= tokens <= 224 (an item's K and V stay in LDS; more tokens are refused, see
 * rart_vit_attention_stream).  (timm Attention.forward; model `vit_base`.) */
int rart_vit_attention(const void* qkv, void* out, int n, int tokens, int heads, int head_dim, rart_stream_t stream);
/* Backward of the same attention (head_dim == 64, 1 <= tokens <= 224): dqkv[n][tokens][3*heads*head_dim] (dQ | dK | dV, qkv's
 * layout) from qkv, the forward's output out[n][tokens][heads*head_dim] and its gradient dout; one fused kernel per
 * (image, head) with Q, K, V and dO resident in LDS, nothing score-sized leaves the chip. */
int rart_vit_attention_bwd(const void* qkv, const void* out, const void* dout, void* dqkv, int n, int tokens, int heads,
                           int head_dim, rart_stream_t stream);
/* The same attention and its backward, STREAMING (csrc/vit_stream.hip): head_dim == 64, any tokens >= 1 (up to 2^20; a shape beyond
 * the kernels' 32-bit indices is refused with a message).  One workgroup per (image, head, block of at most eight 32-query tiles);
 * K / V pass through LDS in chunks of 64 rows under a running maximum and sum per query.  The backward is two launches (query side:
 * dQ and the statistics; key side: dK, dV) and needs stats: scratch of n * heads * 32 * ceil(tokens / 32) * 4 floats (per query:
 * max, 1 / sum, delta).  Layouts are those of the resident entries; the kernels read no row past n*tokens, so the slack rows of qkv
 * may hold anything.  No atomics: results are bit-reproducible and an image's rows do not depend on the batch. */
int rart_vit_attention_stream(const void* qkv, void* out, int n, int tokens, int heads, int head_dim, rart_stream_t stream);
int rart_vit_attention_bwd_stream(const void* qkv, const void* out, const void* dout, void* dqkv, float* stats, int n, int tokens,
                                  int heads, int head_dim, rart_stream_t stream);
/* vt[n][heads][head_dim][t_pad] <- V slice of the fused qkv activation [n][tokens][qkv_ld] (zero padded). */
int rart_vit_transpose_v(const void* qkv, void* vt, int n, int tokens, int heads, int head_dim, int qkv_ld, int v_off,
                         int t_pad, rart_stream_t stream);

/* ViT-B/16 backward-to-input pieces (autograd through timm's VisionTransformer for the attack gradient); the
 * contractions run on rart_conv_igemm_bf16 (batched for the per-head products).  bf16 storage, fp32 math. */
int rart_gelu_bf16(const void* u, void* out, size_t n, rart_stream_t stream);            /* exact (erf) GELU */
int rart_gelu_bwd_bf16(const void* dh, const void* u, void* du, size_t n, rart_stream_t stream);   /* du = dh*gelu'(u) */
/* dx = LayerNorm backward to the input (statistics recomputed from x) [+ res]; strides in elements per row. */
int rart_layernorm_bwd_bf16(const void* dy, const void* x, const float* gamma, const void* res, void* dx, int rows, int dim,
                            int64_t dy_row_stride, int64_t x_row_stride, int64_t res_row_stride, int64_t dx_row_stride,
                            float eps, rart_stream_t stream);
/* dS = scale * P * (dP - rowsum(P*dP)) on [0, n_valid), zeros up to ld_out (soft-max backward, scale = 1/sqrt(head_dim)). */
int rart_softmax_bwd_rows_bf16(const void* probs, const void* dprobs, void* dscores, int64_t rows, int n_valid, int ld_p,
                               int ld_dp, int ld_out, float scale, rart_stream_t stream);
/* grad[b][c][y][x] (fp32, w.r.t. the [0,1] image) from the patch-embedding input gradient [b*patches][ld >= 3*p*p]. */
int rart_vit_unpatchify_f32(const void* dpatches, float* grad, int n, int h, int w, int patch, int64_t ld,
                            const float* std_host, rart_stream_t stream);
/* ViT training: LayerNorm backward to the input (dx nullable) plus dgamma = sum_rows dy*xhat, dbeta = sum_rows dy
 * (written, or added when accumulate != 0); deterministic two-level reduction.  workspace: rart_layernorm_bwd_workspace_bytes. */
size_t rart_layernorm_bwd_workspace_bytes(int dim);
int rart_layernorm_bwd_full_bf16(const void* dy, const void* x, const float* gamma, const void* res, void* dx, int rows,
                                 int dim, int64_t dy_row_stride, int64_t x_row_stride, int64_t res_row_stride,
                                 int64_t dx_row_stride, float eps, float* dgamma, float* dbeta, int accumulate, void* workspace,
                                 size_t workspace_bytes, rart_stream_t stream);
/* out[c] (+)= sum_r x[r][c] for a bf16 [rows][cols] matrix with row stride ld (Linear bias gradients, position embedding). */
size_t rart_colsum_workspace_bytes(int rows, int cols);
int rart_colsum_bf16(const void* x, int64_t ld, int rows, int cols, float* out, int accumulate, void* workspace,
                     size_t workspace_bytes, rart_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Training-side step kernels.  The solver the reference launches
 * (RobustART/train/__init__.py:1 -> absent submodule) is configured by
 * exprs/nips_benchmark/pgd_adv_train/resnet50/config.yaml:11-33 (SGD nesterov 0.9, wd 1e-4, label_smooth 0.1,
 * EMA 0.9999) and exprs/nips_benchmark/new_adv_train/vit_base/config.yaml:11-38 (AdamW); the arithmetic is
 * torch.optim.SGD / torch.optim.AdamW / F.cross_entropy(label_smoothing).  All buffers are flat fp32 arenas,
 * 16-byte aligned, updated in place.
 *   g' = grad*grad_scale (+ weight_decay*param for SGD); grad_scale folds the 1/world_size of the gradient mean.
 *   ema (nullable): ema = ema_decay*ema + (1-ema_decay)*param_new.   zero_grad != 0: grad is reset to 0.
 * Hyper-parameters are doubles (Python floats in the reference's configs); the kernels compute in fp32 and form
 * 1-beta, 1-lr*wd, 1-decay in double rounded once, as torch does with its scalar arguments.
 * ------------------------------------------------------------------------------------- */
int rart_sgd_step_f32(float* param, float* grad, float* momentum_buf, float* ema, size_t n, double lr, double momentum,
                      double weight_decay, int nesterov, double grad_scale, double ema_decay, int zero_grad,
                      rart_stream_t stream);
/* step counts from 1 (bias corrections 1-beta^step); decoupled weight decay (param *= 1 - lr*wd). */
int rart_adamw_step_f32(float* param, float* grad, float* exp_avg, float* exp_avg_sq, float* ema, size_t n, double lr,
                        double beta1, double beta2, double eps, double weight_decay, int step, double grad_scale,
                        double ema_decay, int zero_grad, rart_stream_t stream);
int rart_ema_update_f32(float* ema, const float* param, size_t n, double decay, rart_stream_t stream);
/* loss_out[batch] (nullable) = (1-s)*(-log p_y) + s*mean_c(-log p_c);
 * dlogits_out[batch][classes] (nullable) = scale * (softmax - (1-s)*onehot - s/classes). */
int rart_label_smooth_ce_f32(const float* logits, const int64_t* labels, int batch, int classes, double smoothing,
                             double scale, float* loss_out, float* dlogits_out, rart_stream_t stream);
/* The two-label loss of Mixup / CutMix (`mixup`, `cutmix` of the solver's config; robustart_amd/train/mixing.py), L = the loss above:
 *   loss_out[b] = lam * L(z_b, labels_a[b]) + (1 - lam) * L(z_b, labels_b[b])   (two fp32 products, one fp32 sum)
 *   dlogits_out = scale * (softmax - s/classes - (1-s)*lam*onehot(labels_a) - (1-s)*(1-lam)*onehot(labels_b)), both terms subtracted
 *   where the labels agree.  lam in [0, 1]; lam and 1 - lam are formed in double and rounded to fp32 once.  lam = 1 (0) reproduces
 *   rart_label_smooth_ce_f32 on labels_a (labels_b) bit for bit.  As there, every label must lie in [0, classes): the labels index the
 *   row of logits and are not range-checked on the device (the caller's contract). */
int rart_label_smooth_ce_mix_f32(const float* logits, const int64_t* labels_a, const int64_t* labels_b, int batch, int classes,
                                 double smoothing, double lam, double scale, float* loss_out, float* dlogits_out, rart_stream_t stream);

/* ---- Mixup / CutMix of a batch (csrc/batch_mix.hip; robustart_amd/train/mixing.py) ------------------------------------------------
 * src: uint8 NHWC [n][h][w][3] (src_is_u8 = 1; x01 = u8 * (1 / 255), the arithmetic of rart_u8_to_unit_f32_nchw) or fp32 NCHW
 * [n][3][h][w] in [0, 1] (0).  perm: int32 [n] on the device, every entry in [0, n) (the caller's contract).  dst: fp32 NCHW, out of
 * place (image i is also read as the partner of another image): dst must not overlap src.
 *   mode 1 (Mixup):  dst[i] = lam * x01[i] + (1 - lam) * x01[perm[i]]  (two fp32 products and one fp32 sum, no contraction; lam and
 *                    1 - lam formed in double, rounded to fp32 once)
 *   mode 2 (CutMix): dst[i] = x01[perm[i]] for y0 <= y < y1 and x0 <= x < x1, x01[i] elsewhere; lam is not used.
 * 0 <= y0 <= y1 <= h, 0 <= x0 <= x1 <= w, 0 <= lam <= 1, n * 3 * h * w < 2^32.  16 bytes per store when w % 4 == 0 and the pointers
 * allow it (dst 16-byte aligned, src 4-byte (u8) / 16-byte (fp32) aligned), one element per thread otherwise, with identical results. */
int rart_mix_batch_f32(const void* src, int src_is_u8, const int32_t* perm, float* dst, int n, int h, int w, int mode, double lam,
                       int y0, int y1, int x0, int x1, rart_stream_t stream);

/* ---- ColorJitter of a batch (csrc/color_jitter.hip; robustart_amd/train/jitter.py) -----------------------------------------------------
 * torchvision's ColorJitter on PIL images is a chain of Pillow calls; this entry computes the same bytes on uint8 NHWC [n][h][w][3].
 * One record per sample: up to four operations in application order,
 *   0 brightness  Image.blend(black, img, factor[0])           1 contrast    Image.blend(grey(m), img, factor[1]), m = int(mean(L) + 0.5)
 *   2 saturation  Image.blend(L as RGB, img, factor[2])        3 hue         RGB -> HSV, H += hue_shift (mod 256), HSV -> RGB
 * with Pillow's convert('L'), blend (fp32, product and sum rounded separately, clamped, truncated) and HSV conversions; the contrast
 * mean is taken of the image as the operations before it left it.  An id outside 0..3, or one that an earlier slot of the record already
 * carries, skips the slot; a record of four skips copies the sample.  The records live on the device and are not inspected by the
 * host: the caller validates them before the upload (robustart_amd/train/jitter.py, pack_jitter). */
typedef struct rart_jitter_rec {
  uint8_t op[4];      /* operation ids in application order */
  float factor[3];    /* blend factors of brightness, contrast, saturation (indexed by id), >= 0 */
  uint32_t hue_shift; /* 0..255 */
} rart_jitter_rec;    /* 20 bytes, no padding */
/* dst == src (in place) or disjoint buffers; any other overlap is refused.  params: n records on the device.  lsum: n words of device
 * workspace (the per-sample luminance sums of the contrast mean); the entry clears it on `stream` itself.  h * w <= 2^24 (the 32-bit
 * luminance sum), n * h * w * 3 < 2^32.  Two launches: the luminance sums of the samples with a contrast slot, then every slot per pixel. */
int rart_color_jitter_u8(const uint8_t* src, uint8_t* dst, int n, int h, int w, const void* params, uint32_t* lsum, rart_stream_t stream);

/* ---- Prediction / confidence / correctness over a class subset (csrc/logit_confidence.hip; robustart_amd/metrics/confidence.py) -----
 * What the ImageNet-A / ImageNet-O evaluation keeps of a sample.  logits: fp32 [rows][ld], ld >= classes, no row alignment assumed.
 * subset: n_subset class indices on the device, each in [0, classes) (NOT range-checked on the device: the caller's contract, as for
 * the labels of rart_label_smooth_ce_f32); NULL or n_subset == 0 selects all classes.  K = the number of selected classes, z = the K
 * selected logits of a row in subset order:
 *   pred[r]    = the LOWEST position in [0, K) that attains max z: a subset coordinate, the label an image-folder dataset over the
 *                subset's class folders gives its samples
 *   conf[r]    = 1 / sum_j expf(z_j - max z), the largest soft-max probability over the subset: fp32, accurate expf, IEEE division
 *   correct[r] = pred[r] == labels[r] (int64, subset coordinates; a label outside [0, K) gives 0); labels == NULL writes 0 everywhere
 *                (the out-of-distribution set)
 * Special values: a -inf entry contributes 0; if any selected logit is NaN, conf is NaN and pred the position of the first NaN
 * (numpy.argmax); a +inf logit or a row of -inf only gives conf = NaN and pred = the first position of the maximum.
 * One launch, no workspace, no atomics; rows are walked with a grid stride (rows is 64-bit) and K has no ceiling (K <= 1024 is held in
 * registers, larger K loops over the row twice).  A row's three outputs depend on its K values alone: they are bit-identical whatever
 * else the launch holds.  rows == 0 returns RART_OK and launches nothing; rows < 0, classes < 1, ld < classes, n_subset outside
 * [0, classes] or a NULL logits / pred / conf / correct with rows > 0 is RART_ERR_INVALID, decided before any HIP call. */
int rart_logit_confidence_f32(const float* logits, int64_t rows, int classes, int64_t ld, const int32_t* subset, int n_subset,
                              const int64_t* labels, int32_t* pred, float* conf, uint8_t* correct, rart_stream_t stream);

/* ---- Prediction, label rank and top-k hit counters (csrc/topk_score.hip; robustart_amd/metrics/confidence.py: topk_score) ----------
 * What the ImageNet-C loop keeps of a batch.  logits: fp32 [rows][ld], ld >= classes, no alignment assumed (16-byte loads are used
 * when the base is 16-byte aligned and ld a multiple of 4, element loads otherwise).  labels: int64 [rows] on the device.  With
 * y = labels[r] and z the first `classes` values of row r:
 *   rank[r] = #{j : z_j > z_y} + #{j < y : z_j == z_y}: the position of the label in a stable descending sort of z, ties to the lower
 *             class index (what torch.topk(sorted) returns on the CPU and metrics.evaluators._topk_acc restates).  A label outside
 *             [0, classes) or a NaN z_y gives rank = classes.  The compares are IEEE: a NaN elsewhere never outranks the label, +inf
 *             and -inf need no special case.
 *   pred[r] = the LOWEST index that attains max z; if the row holds a NaN, the index of the first NaN (numpy.argmax, the rule of
 *             rart_logit_confidence_f32)
 *   hits[i] += #{r : rank[r] < ks[i] and rank[r] < classes} for i < n_k, 0 <= n_k <= 8: rank = classes is a miss for EVERY k, also
 *             for a k above classes.  ks: HOST array, copied into the launch arguments, every entry >= 1.  hits: int64 on the DEVICE;
 *             the entry ADDS and never clears (the caller passes hits + 2 * slot to keep a pair of counters per slot), with one
 *             64-bit atomic add per workgroup and k after a register + LDS reduction.  The sums are integers: no order dependence.
 * pred, rank and hits may each be NULL to skip that output (hits == NULL or n_k == 0 skips the counting).  One launch, no workspace;
 * one wave per row, rows (64-bit) walked with a grid stride of at most 8192 rows per trip; a row is read once whatever `classes` is
 * (no ceiling).  A row's pred and rank depend on that row alone.  rows == 0 returns RART_OK and launches nothing; rows < 0,
 * classes < 1, ld < classes, n_k outside [0, 8], NULL ks with n_k > 0, a ks[i] < 1, or NULL logits / labels with rows > 0 is
 * RART_ERR_INVALID, decided before any HIP call. */
int rart_topk_score_f32(const float* logits, int64_t rows, int classes, int64_t ld, const int64_t* labels, int32_t* pred, int32_t* rank,
                        const int* ks, int n_k, int64_t* hits, rart_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Train-mode conv + BatchNorm support (cls_solver training step): the contractions run on
 * rart_conv_igemm_bf16; these are the HBM-bound kernels around it.  Activations are bf16 [rows][channels]
 * (NHWC, rows = batch*h*w), statistics fp32.  channels: a power of two in [8, 2048].
 * Reference arithmetic: torch.nn.BatchNorm2d (training mode) and conv2d's autograd.
 * ------------------------------------------------------------------------------------- */
size_t rart_bn_workspace_bytes(size_t rows, int channels);
/* batch statistics of z, y = [relu](z*scale + shift [+ res]); running stats updated in place when non-NULL
 * (running_var with the unbiased variance); mean_out / invstd_out [channels] are kept for the backward;
 * scale_shift [2][channels] receives gamma*invstd and beta - mean*gamma*invstd.  sign_out (nullable): [rows][channels / 8] bytes,
 * bit j of byte (row, c / 8) = (y[row][c] > 0): the backward's ReLU mask at 1/16 of y's bytes.  stats_partial (nullable):
 * [stats_chunks][2][channels] fp32 column sums / sums of squares of z from the producing convolution (rart_conv_desc.bn_stats_out)
 * -- then no statistics pass reads z. */
int rart_bn_train_forward_bf16(const void* z, const void* res, void* y, void* sign_out, size_t rows, int channels, const float* gamma,
                               const float* beta, float* running_mean, float* running_var, double momentum, double eps,
                               int relu, float* mean_out, float* invstd_out, float* scale_shift, const float* stats_partial,
                               int stats_chunks, void* workspace, size_t workspace_bytes, rart_stream_t stream);
/* g = dy * [ymask > 0] (ymask NULL: g = dy; ymask_is_bits: ymask is the forward's sign_out instead of the bf16 activation);
 * dgamma = sum g*xhat, dbeta = sum g (written, or added when accumulate != 0); dz = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat));
 * g_out (nullable) receives g.  coef: [3][channels] fp32 scratch. */
int rart_bn_train_backward_bf16(const void* dy, const void* ymask, int ymask_is_bits, const void* z, void* dz, void* g_out, size_t rows,
                                int channels, const float* gamma, const float* mean, const float* invstd, float* dgamma,
                                float* dbeta, int accumulate, float* coef, void* workspace, size_t workspace_bytes,
                                rart_stream_t stream);
/* T[(t*channels + c)][m] = src[img(m), oy*sy + tap_dy[t], ox*sx + tap_dx[t], c] for m < batch*grid_h*grid_w, zero
 * outside the image and for the padding up to rows_padded (multiple of 64): the K(=pixel)-contiguous operand of the
 * weight-gradient GEMM.  Stored as one compact slab per K split, dst[m / chunk][row][m % chunk] with rows_total rows
 * per slab (chunk 0 = a single slab; rows_total 0 = taps*channels): a split then touches a few MB instead of one
 * 128-byte piece from each of hundreds of multi-MB rows (TLB / DRAM-page locality).
 * channels: 4 (stem's padded plane) or a multiple of 8. */
int rart_transpose_gather_bf16(const void* src, void* dst, int batch, int src_h, int src_w, int channels, int grid_h,
                               int grid_w, int sy, int sx, int n_taps, const int* tap_dy, const int* tap_dx,
                               long long rows_padded, int chunk, int rows_total, rart_stream_t stream);
/* Weight gradient straight from the NHWC activations (csrc/wgrad_direct.hip): partial[z][t * channels + c][n] = sum over the positions m of
 * K split z (chunk positions each) of x[pixel(m) + tap t][c] * dz[m][n], fp32, the layout rart_wgrad_reduce_f32 folds -- without the two
 * rart_transpose_gather_bf16 passes: the position-major tiles are read out of LDS transposed (ds_read_b64_tr_b16).  x [batch][in_h][in_w]
 * [channels], dz [batch][grid_h][grid_w][dz_cols] bf16; channels 64 or a multiple of 128, dz_cols a multiple of 64, 1..9 taps -- or
 * channels 4 (the stem's padded plane: 32 taps x 4 channels per tile, 4-byte direct loads), dz_cols 64, 1..49 taps;
 * chunk a multiple of 32 with splits * chunk >= batch * grid_h * grid_w; ld_n = dz_cols.  (loss.backward() of cls_solver.py:183-215) */
int rart_wgrad_direct_supported(int channels, int dz_cols, int n_taps);
int rart_wgrad_direct_bf16(const void* x, const void* dz, float* partial, int batch, int in_h, int in_w, int channels, int grid_h, int grid_w,
                           int dz_cols, int stride_y, int stride_x, int n_taps, const int* tap_dy, const int* tap_dx, int splits, int chunk,
                           int ld_n, rart_stream_t stream);
/* grad[n][c][t] (torch conv weight layout, t = r*S + s) (+)= sum_z partial[z][t*channels_padded + c][n];
 * partial: fp32 [splits][taps*channels_padded][ld_n], the split-K output of rart_conv_igemm_bf16; it is scratch:
 * more than 16 splits are first folded 16:1 in place. */
int rart_wgrad_reduce_f32(float* partial, int splits, int taps, int channels, int channels_padded, int n_out,
                          int ld_n, float* grad, int accumulate, rart_stream_t stream);
/* fp32 master weight [n_out][channels][r][s] -> bf16 igemm table over the listed taps:
 * transpose 0: out[n][ti*channels + c] (forward), 1: out[c][ti*n_out + n] (backward to input); rows zero-padded.
 * out_channel_scale (nullable, [n_out]): weight[n] is multiplied by it first -- the eval-mode BatchNorm fold
 * gamma*rsqrt(running_var + eps), so the attack engine can be re-folded from the live parameters every iteration. */
int rart_pack_conv_weight_bf16(const float* weight, const float* out_channel_scale, void* out, int n_out, int channels,
                               int r, int s, int n_taps, const int* tap_r, const int* tap_s, int transpose,
                               int rows_padded, rart_stream_t stream);
/* Many table jobs in ONE launch: the adversarial-training step (cifar10/code/train.py:96-127: attack the CURRENT weights, then update
 * them) re-packs every conv table of the train engine and re-folds every table of the attack engine after each optimizer step -- about
 * 500 launches of 2-10 us kernels.  kind 0 = the job of rart_pack_conv_weight_bf16 (weight / scale / out and the geometry; <= 16 taps),
 * kind 1 = the job of rart_pack_frag_bf16 (src16 -> out, rows x k).  jobs_device: an array of rart_pack_job in DEVICE memory, built once
 * by the caller (every pointer in it must stay valid); blocks_per_job workgroups walk each job grid-strided. */
typedef struct rart_pack_job {
  int kind, n_out, channels, r, s, n_taps, transpose, rows_padded, rows, k;
  int tap_r[16], tap_s[16];
  const float* weight;
  const float* out_channel_scale;
  const void* src16;
  void* out;
} rart_pack_job;
int rart_pack_jobs_bf16(const rart_pack_job* jobs_device, int n_jobs, int blocks_per_job, rart_stream_t stream);

/* ---- ConvNeXt-B (model `convnext_base`, csrc/convnext.hip; robustart_amd/model/convnext_engine.py) ---------------------------------
 * Activations NHWC [n][h][w][c].  *_bf16: bf16 tensors; *_pair: PAIRS of bf16 planes (value = hi + lo, see rart_gemm_pair_bf16), given as
 * explicit hi / lo pointers.  fp32 arithmetic in both.  Reference: timm's ConvNeXt block (robustart_amd/model/convnext_torch.py).
 * rart_cnx_dwconv_ln_*: out = LayerNorm_c(depthwise 7x7 pad 3 convolution of x + b_dw) * gamma + beta (eps), the conv output y kept in
 *   y_keep / y_hi, y_lo (nullable: the backward's LayerNorm input).  w_dw: fp32 [49][c], row dy * 7 + dx = weight[c][0][dy][dx].
 *   One workgroup per (image, row), the row's conv outputs in LDS: c % 8 == 0, c <= 1024, w * c <= 16384, n, h <= 65535; x must not
 *   alias out; activation pointers 8-byte, w_dw / b_dw 16-byte aligned. */
int rart_cnx_dwconv_ln_bf16(const void* x, const float* w_dw, const float* b_dw, const float* gamma, const float* beta, void* out,
                            void* y_keep, int n, int h, int w, int c, float eps, rart_stream_t stream);
int rart_cnx_dwconv_ln_pair(const void* x_hi, const void* x_lo, const float* w_dw, const float* b_dw, const float* gamma, const float* beta,
                            void* out_hi, void* out_lo, void* y_hi, void* y_lo, int n, int h, int w, int c, float eps, rart_stream_t stream);
/* rart_cnx_dwconv_bwd_*: the depthwise convolution's backward to the input, dx = res + sum over taps of dz at (y + 3 - dy, x + 3 - dx)
 *   times w_dw[dy * 7 + dx] (res nullable, may alias dx; dz must not).  dz is the LayerNorm backward's output (rart_layernorm_bwd_*
 *   of the fc1 input gradient against y_keep).  Shape limits as the forward. */
int rart_cnx_dwconv_bwd_bf16(const void* dz, const float* w_dw, const void* res, void* dx, int n, int h, int w, int c, rart_stream_t stream);
int rart_cnx_dwconv_bwd_pair(const void* dz_hi, const void* dz_lo, const float* w_dw, const void* res_hi, const void* res_lo, void* dx_hi,
                             void* dx_lo, int n, int h, int w, int c, rart_stream_t stream);
/* rart_cnx_pool_bwd_*: dz[b][p][c] = dpool[b][c] / hw, the global average pool's backward (no ReLU mask; c % 8 == 0). */
int rart_cnx_pool_bwd_bf16(const void* dpool, void* dz, int n, int hw, int c, rart_stream_t stream);
int rart_cnx_pool_bwd_pair(const void* dpool_hi, const void* dpool_lo, void* dz_hi, void* dz_lo, int n, int hw, int c, rart_stream_t stream);
/* rart_cnx_patchify: src fp32 NCHW in [0,1] (src_is_u8 = 0) or uint8 NHWC (1) -> (x - mean) / std as hi and lo bf16 planes
 *   [n][(h / patch) * (w / patch)][ld], column c * patch^2 + r * patch + s; columns 3 patch^2 .. ld are zero (the stem's K padded to the
 *   GEMM granularity).  patch 1..8 dividing h and w, ld % 8 == 0.  (rart_vit_patchify keeps its patch % 8 == 0 rule.)  The matching
 *   backward is rart_vit_unpatchify_from_f32 with the same patch and ld. */
int rart_cnx_patchify(const void* src, int src_is_u8, void* hi, void* lo, int n, int h, int w, int patch, int ld, const float* mean_host,
                      const float* std_host, rart_stream_t stream);

/* ---- ConvStem (csrc/convstem.hip; robustart_amd/model/convstem_engine.py): the overlapping-convolution stem of `convnext_base_cvst`
 * and `vit_base_cvst`, units of Conv2d(3x3, stride 2, padding 1) -> LayerNorm over channels -> exact GELU.  The convolutions run on
 * rart_conv_igemm_bf16 / rart_gemm_pair_bf16; these are the kernels between them.
 * rart_cvst_im2col: src fp32 NCHW in [0,1] (src_is_u8 = 0) or uint8 NHWC (1) -> the 3x3 / stride-2 / padding-1 patch matrix of the
 *   normalised image (x - mean) / std as bf16 planes hi and lo (lo nullable) [n * (h / 2) * (w / 2)][ld], column c * 9 + ky * 3 + kx
 *   (the Conv2d weight's order); a tap outside the image is 0 (zero padding of the NORMALISED image) and columns 27 .. ld are zero: every
 *   byte of the output is written.  ld % 8 == 0, ld >= 32.  RART_ERR_UNSUPPORTED for an odd h or w.
 * rart_cvst_col2im_f32: the backward: fp32 dpatches [n * (h / 2) * (w / 2)][ld] (27 valid columns) -> grad [n][3][h][w] =
 *   d(loss)/d(x01) including 1 / std.  Every pixel gathers the one, two or four patch entries that cover it in a fixed order (no
 *   atomics, deterministic, every pixel written).  RART_ERR_UNSUPPORTED for an odd h or w.
 * rart_ln_gelu_*: out[r][0 .. dim) = GELU(LayerNorm(x[r][0 .. dim)) * gamma + beta) (exact erf GELU), out[r][dim .. out_row_stride) = 0.
 *   Rows in_row_stride / out_row_stride elements apart (multiples of 8, >= dim); dim 32 .. 1024 in steps of 16; 16-byte aligned
 *   pointers; out must not alias x.
 * rart_ln_gelu_bwd_*: dx[r][0 .. dim) = LayerNorm'(x)^T (dy * GELU'(LayerNorm(x) * gamma + beta)) with the statistics recomputed from
 *   x (the forward's input, i.e. the kept convolution output); dx[r][dim .. dx_row_stride) = 0.  No parameter gradients. */
int rart_cvst_im2col(const void* src, int src_is_u8, void* hi, void* lo, int n, int h, int w, int ld, const float* mean_host,
                     const float* std_host, rart_stream_t stream);
int rart_cvst_col2im_f32(const float* dpatches, float* grad, int n, int h, int w, int ld, const float* std_host, rart_stream_t stream);
int rart_ln_gelu_bf16(const void* x, const float* gamma, const float* beta, void* out, int rows, int dim, int64_t in_row_stride,
                      int64_t out_row_stride, float eps, rart_stream_t stream);
int rart_ln_gelu_pair(const void* x_hi, const void* x_lo, const float* gamma, const float* beta, void* out_hi, void* out_lo, int rows,
                      int dim, int64_t in_row_stride, int64_t out_row_stride, float eps, rart_stream_t stream);
int rart_ln_gelu_bwd_bf16(const void* dy, const void* x, const float* gamma, const float* beta, void* dx, int rows, int dim,
                          int64_t dy_row_stride, int64_t x_row_stride, int64_t dx_row_stride, float eps, rart_stream_t stream);
int rart_ln_gelu_bwd_pair(const void* dy_hi, const void* dy_lo, const void* x_hi, const void* x_lo, const float* gamma, const float* beta,
                          void* dx_hi, void* dx_lo, int rows, int dim, int64_t dy_row_stride, int64_t x_row_stride, int64_t dx_row_stride,
                          float eps, rart_stream_t stream);

/* ---- ConvNeXt-B training (csrc/convnext_train.hip; robustart_amd/model/convnext_train_engine.py), bf16 storage, fp32 arithmetic -------
 * rart_cnx_dwconv_wgrad_bf16: the 7x7 pad-3 depthwise convolution's weight and bias gradient, dw[dy * 7 + dx][c] (+)= sum over
 *   (image, y, x) of x[y + dy - 3][x + dx - 3][c] * dz[y][x][c] and db[c] (+)= sum dz (accumulate != 0 adds).  x: the block input, dz: the
 *   gradient of the conv output, both NHWC [n][h][w][c] bf16.  dw_layout 0: dw is [49][c] (the w_dw layout of rart_cnx_dwconv_ln_*),
 *   1: [c][49] (the module's conv_dw.weight [c][1][7][7]).  Deterministic: fp32 per-workgroup partials in `workspace`
 *   (rart_cnx_dwconv_wgrad_workspace_bytes, 0 for an unsupported shape), folded in a fixed order.  c % 8 == 0, c <= 1024, w <= 128,
 *   n, h <= 65535; x / dz 8-byte aligned. */
size_t rart_cnx_dwconv_wgrad_workspace_bytes(int n, int h, int w, int c);
int rart_cnx_dwconv_wgrad_bf16(const void* x, const void* dz, float* dw, float* db, int n, int h, int w, int c, int dw_layout, int accumulate,
                               void* workspace, size_t workspace_bytes, rart_stream_t stream);
/* rart_cnx_layer_scale_fwd_bf16: x_out = x_in + gamma * u2 over bf16 [rows][c] (u2 = the block's unscaled fc2 output, kept for the
 *   backward; x_out may alias x_in, not u2).
 * rart_cnx_layer_scale_bwd_bf16: from dx (the gradient of the block output) and u2: dv = gamma * dx (bf16, fc2's output gradient),
 *   dgamma[c] (+)= sum_rows dx * u2 and, when db2 is non-null, db2[c] (+)= sum_rows gamma * dx (fc2's bias gradient) in the same pass.
 *   Deterministic like the weight gradient; workspace: rart_cnx_layer_scale_bwd_workspace_bytes.  gamma is never divided out.
 *   Both: c % 8 == 0, c <= 1024, 0 < rows < 2^31; bf16 pointers 16-byte aligned; dv must not alias dx or u2. */
int rart_cnx_layer_scale_fwd_bf16(const void* x_in, const void* u2, const float* gamma, void* x_out, long long rows, int c, rart_stream_t stream);
size_t rart_cnx_layer_scale_bwd_workspace_bytes(long long rows, int c);
int rart_cnx_layer_scale_bwd_bf16(const void* dx, const void* u2, const float* gamma, void* dv, float* dgamma, float* db2, long long rows,
                                  int c, int accumulate, void* workspace, size_t workspace_bytes, rart_stream_t stream);

/* ---- ConvNeXt-V2-B Global Response Norm (model `convnextv2_base`, csrc/convnext_v2.hip; robustart_amd/model/convnext_engine.py) ------
 * y: the GELU output of a block's fc1, per image [p][c] (p = h * w pixels, c = the hidden width); *_bf16 / *_pair as above, fp32
 *   arithmetic and statistics.  G, a: fp32 [n][c].  w, b: mlp.grn.weight / bias, fp32 [c].  m = mean_c G[n][c].
 * rart_cnx_grn_stats_*: G[n][c] = sqrt(sum_p y^2).
 * rart_cnx_grn_apply_*: z = y * (1 + w[c] * G[n][c] / (m + eps)) + b[c]; z may alias y (both planes of it) or be another buffer.
 * rart_cnx_grn_bwd_reduce_*: a[n][c] = w[c] * sum_p g * y, g = the gradient of z.
 * rart_cnx_grn_bwd_apply_*: dh = (g * (1 + w[c] G[c] / (m + eps)) + y * beta[c] / G[c]) * gelu'(u), beta[c] = a[c] / (m + eps) -
 *   s / (c * (m + eps)^2), s = sum_c a[c] G[c] (the y term 0 where G[c] == 0); u = the fc1 pre-activation (exact-erf GELU).  dh may
 *   alias g (both planes), not y or u.
 * Deterministic, no atomics: a reduction over pixels is one workgroup per (image, 128 channels), the per-image scalars are fixed-order
 *   block sums, and no launch geometry depends on n.  c % 8 == 0, c <= 4096, 0 < n <= 65535, p > 0; bf16 pointers 16-byte aligned. */
int rart_cnx_grn_stats_bf16(const void* y, float* G, int n, int p, int c, rart_stream_t stream);
int rart_cnx_grn_stats_pair(const void* y_hi, const void* y_lo, float* G, int n, int p, int c, rart_stream_t stream);
int rart_cnx_grn_apply_bf16(const void* y, const float* G, const float* w, const float* b, void* z, int n, int p, int c, float eps,
                            rart_stream_t stream);
int rart_cnx_grn_apply_pair(const void* y_hi, const void* y_lo, const float* G, const float* w, const float* b, void* z_hi, void* z_lo, int n,
                            int p, int c, float eps, rart_stream_t stream);
int rart_cnx_grn_bwd_reduce_bf16(const void* g, const void* y, const float* w, float* a, int n, int p, int c, rart_stream_t stream);
int rart_cnx_grn_bwd_reduce_pair(const void* g_hi, const void* g_lo, const void* y_hi, const void* y_lo, const float* w, float* a, int n, int p,
                                 int c, rart_stream_t stream);
int rart_cnx_grn_bwd_apply_bf16(const void* g, const void* y, const void* u, const float* G, const float* a, const float* w, void* dh, int n,
                                int p, int c, float eps, rart_stream_t stream);
int rart_cnx_grn_bwd_apply_pair(const void* g_hi, const void* g_lo, const void* y_hi, const void* y_lo, const void* u_hi, const void* u_lo,
                                const float* G, const float* a, const float* w, void* dh_hi, void* dh_lo, int n, int p, int c, float eps,
                                rart_stream_t stream);
/* rart_cnx_grn_bwd_reduce_train_bf16 (ConvNeXt-V2 training, bf16 only): rart_cnx_grn_bwd_reduce_bf16 plus GRN's parameter gradients in
 *   the same pass over g and y:  a[n][c] = w[c] * sum_p g * y (the same bits as rart_cnx_grn_bwd_reduce_bf16),
 *   dw[c] (+)= sum_n N[n][c] * sum_p g * y,  db[c] (+)= sum_n sum_p g,  N[n][c] = G[n][c] / (m + eps)  (accumulate != 0 adds).
 *   G: the forward's rart_cnx_grn_stats_bf16 output; m + eps is formed with rart_cnx_grn_apply_bf16's fixed-order block sum, so N is
 *   the forward's.  Deterministic, no atomics: per-image fp32 partials in `workspace` (rart_cnx_grn_param_grad_workspace_bytes, 0 for
 *   an unsupported shape), folded over n in a fixed order.  Shape and alignment rules as above. */
size_t rart_cnx_grn_param_grad_workspace_bytes(int n, int c);
int rart_cnx_grn_bwd_reduce_train_bf16(const void* g, const void* y, const float* G, const float* w, float* a, float* dw, float* db, int n,
                                       int p, int c, float eps, int accumulate, void* workspace, size_t workspace_bytes,
                                       rart_stream_t stream);

/* Token-mixing GEMM of MLP-Mixer (csrc/mixer.hip): per image b of `batch`,
 *   C_b[m][n] = sum_k A[m][k] X_b[k][n]     (m < M, n < N, k < K; fp32 accumulation)
 * a_*: the weight table [M][lda], K contiguous, shared by every image; lda >= K rounded up to 32 and a multiple of 8, columns K .. lda - 1
 *   zero.  x_*: image b's activation slab [K][ldx] (n contiguous) at element b * x_stride; rows k >= K are never read (zeros instead).
 * dst_*: image b's [M][ldc] at element b * c_stride; res_* (indexed like dst, may alias it), aux_* (likewise).  bias: fp32 [M] or null.
 * The epilogue (fp32): + bias[m]; + res; then flag 4 = GELU (of the value rounded to the output format of u), 64 = the same GELU with u
 * written to aux, 8 = times gelu'(aux); flag 2 = fp32 output (dst_hi as float*).  rart_tokmix_bf16: bf16 planes (the *_lo are unused);
 * rart_tokmix_pair: hi + lo bf16 planes of A, X, res, aux and dst, three MFMA products hi.hi + hi.lo + lo.hi per contraction (the
 * arithmetic of rart_gemm_pair_bf16).  N, ldx, x_stride: multiples of 8; A and X planes 16-byte aligned.  No result depends on the batch. */
typedef struct rart_tokmix_desc {
  const void *a_hi, *a_lo, *x_hi, *x_lo;
  void *dst_hi, *dst_lo;
  const void *res_hi, *res_lo;
  void *aux_hi, *aux_lo;
  const float* bias;
  int M, N, K, lda, ldx, ldc, batch, flags;
  int64_t x_stride, c_stride;
} rart_tokmix_desc;
int rart_tokmix_bf16(const rart_tokmix_desc* desc, rart_stream_t stream);
int rart_tokmix_pair(const rart_tokmix_desc* desc, rart_stream_t stream);

/* Gradient of a token-mixing weight table (csrc/mixer_train.hip, bf16 training):
 *   G[m][n] = sum_b sum_d P_b[m][d] Q_b[n][d]     (m < M, n < N, d < D, b < batch; bf16 operands, fp32 accumulation)
 * p / q: per-image slabs [M][D] / [N][D], D contiguous, image b at element b * p_stride / b * q_stride; 16-byte aligned, D and the
 *   strides multiples of 8, p_stride >= M D, q_stride >= N D.  Rows past M / N and channels past D are never read (zeros instead).
 * Split z < splits sums images [z * images_per_split, (z + 1) * images_per_split) (splits * images_per_split >= batch) into
 * partial[z][n][m], fp32 [splits][N][ld_partial >= M]: the layout rart_wgrad_reduce_f32(partial, splits, 1, N, N, M, ld_partial, grad, ..)
 * folds into grad[M][N], the torch layout of the table (dW1: P = d(u_tok), Q = LN1(x); dW2: P = dx', Q = gelu(u_tok)).
 * Fixed summation order, no atomics: the same bits on every run. */
typedef struct rart_tokmix_wgrad_desc {
  const void *p, *q;
  float* partial;
  int M, N, D, batch, splits, images_per_split, ld_partial, reserved;
  int64_t p_stride, q_stride;
} rart_tokmix_wgrad_desc;
int rart_tokmix_wgrad_bf16(const rart_tokmix_wgrad_desc* desc, rart_stream_t stream);
/* out[m] (+)= sum_b sum_d x[b][m][d] for bf16 per-image slabs [rows][dim] `stride` elements apart (the token biases' gradients; dim and
 * stride multiples of 8, stride >= rows dim, x 16-byte aligned); deterministic two-level reduction.
 * workspace: rart_tok_rowsum_workspace_bytes(rows, batch). */
size_t rart_tok_rowsum_workspace_bytes(int rows, int batch);
int rart_tok_rowsum_bf16(const void* x, int rows, int dim, int batch, int64_t stride, float* out, int accumulate, void* workspace,
                         size_t workspace_bytes, rart_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * JPEG reader (csrc/jpeg_entropy.h + csrc/jpeg_decode.hip): Image.open(f).convert('RGB') of the reference's 'pil' reader
 * (imagenet_s_gen.py:177-196) split the way its DALI reader splits it (pgd_adv_train/resnet50/config.yaml:38) -- entropy decoding
 * on the host, the arithmetic on the device -- and bit-exact with Pillow / libjpeg-turbo.
 *
 * Supported set: baseline SOF0, 8-bit samples and quantisation tables, one scan; grayscale, or three components with chroma (1,1)
 * and luma (1,1) / (2,1) / (2,2) read as YCbCr (a JFIF APP0, or an Adobe APP14 with transform 1, or no Adobe marker and ids 1,2,3);
 * restart intervals, optimised Huffman tables, fill bytes and FF00 stuffing included.  Any other file (progressive, SOF1,
 * arithmetic, lossless, 12-bit, DNL, 16-bit tables, 4:4:0, CMYK, several scans, more than 2^26 pixels, not a JPEG) gives
 * RART_ERR_UNSUPPORTED; a supported file with a truncated or corrupt stream gives RART_ERR_INVALID.
 *
 * rart_jpeg_probe / rart_jpeg_entropy_decode are HOST-ONLY (every pointer is a host pointer, no HIP call, safe from any number of
 * threads at once).  probe fills `info` (info->status repeats the return value).  entropy_decode writes the coefficients of the
 * scan to coef_host: per component, block-row-major over the MCU-padded block grid blocks_h x blocks_w, 64 int16 per block in
 * natural (de-zigzagged) order, not dequantised; `capacity` counts int16 elements.  Unless it returns RART_OK or RART_ERR_INVALID
 * coef_host is not written. */
typedef struct rart_jpeg_info {
  int32_t status;                 /* RART_OK: in the supported set */
  int32_t height, width, ncomp;   /* ncomp 1 or 3 */
  int32_t h_samp[3], v_samp[3];
  int32_t blocks_w[3], blocks_h[3];   /* the MCU-padded block grid of each component */
  int64_t coef_count;             /* 64 * the sum of the blocks */
  uint16_t qt[3][64];             /* each component's quantisation table, natural order */
} rart_jpeg_info;
int rart_jpeg_probe(const uint8_t* data_host, size_t len, rart_jpeg_info* info_host);
int rart_jpeg_entropy_decode(const uint8_t* data_host, size_t len, const rart_jpeg_info* info_host, int16_t* coef_host,
                             size_t capacity);

/* The device stage: dequantise + ISLOW IDCT (jidctint.c: idct8<11> over columns, idct8<18> over rows, + 128, clamp) into uint8
 * component planes in the workspace (row stride 8 blocks_w), then libjpeg's upsampling (fancy h2v1 / h2v2 triangle filters; plain
 * replication when the chroma plane is at most 2 samples wide; indices clamped to the component's real extent
 * ceil(w h_samp / h_max) x ceil(h v_samp / v_max)) + YCbCr -> RGB into `out`, uint8 [height][width][3] per image, packed back to
 * back.  Two launches for the whole batch, whatever n and however the images differ.
 * One descriptor per image, in batch order; the batch's blocks are numbered image by image, component by component, block-row-major:
 *   block_start[c] : number of component c's first block (absent components: the next image's first); its coefficients start
 *                    at element 64 block_start[c] of `coef`.  Image 0 starts at 0, nothing is skipped.
 *   qt_off         : element of `qt` (uint16) where the image's [3][64] tables start (natural order), a multiple of 8
 *   plane_off[c]   : byte of the workspace where component c's plane starts, a multiple of 16
 *   out_off        : byte of `out` where the image starts = 3 * the pixels of the images before it
 *   h_samp, v_samp : luma's sampling factors (chroma is (1,1)); 1 / 1 for grayscale
 * desc and desc_host hold the same n descriptors on the device and on the host: the host copy is validated against
 * total_blocks / qt_count / workspace_bytes / out_bytes BEFORE any launch (RART_ERR_INVALID, RART_ERR_WORKSPACE), so a descriptor
 * cannot make a kernel write outside the caller's buffers.  coef: total_blocks * 64 int16, 16-byte aligned. */
typedef struct rart_jpeg_desc {
  int64_t block_start[3];
  int64_t plane_off[3];
  int64_t qt_off, out_off;
  int32_t height, width, ncomp, h_samp, v_samp;
  int32_t blocks_w[3], blocks_h[3];
  int32_t reserved_;
} rart_jpeg_desc;
size_t rart_jpeg_decode_workspace_bytes(const rart_jpeg_desc* desc_host, int n);
int rart_jpeg_decode_u8(const rart_jpeg_desc* desc, const rart_jpeg_desc* desc_host, int n, const int16_t* coef, int64_t total_blocks,
                        const uint16_t* qt, size_t qt_count, void* workspace, size_t workspace_bytes, uint8_t* out, size_t out_bytes,
                        rart_stream_t stream);

/* Entropy decoding on the device (csrc/jpeg_entropy_par.h + csrc/jpeg_entropy_gpu.hip): a self-synchronising
 * parallel Huffman decoder, one workgroup per image, whose coefficients are those of rart_jpeg_entropy_decode element for
 * element.  The scan is cut into subsequences of subseq_bytes raw bytes (a power of two from 4 up; 0 = the default); all of them
 * decode from a guessed state, then rounds re-decode those whose entry changed until a round changes nothing; prefix sums over the
 * subsequences place the blocks and the DC predictors, and a last pass writes the coefficients.  An image that has not converged
 * after max_rounds rounds (0 = the default) gets status RART_ERR_UNSUPPORTED ("decode it with rart_jpeg_entropy_decode"), a
 * truncated or corrupt stream RART_ERR_INVALID, exactly where rart_jpeg_entropy_decode returns it; never a guess.
 *
 * rart_jpeg_scan_plan is HOST-ONLY.  From a file and its probe it fills *scan_host -- all but the four offsets the caller owns --
 * and writes the image's distinct Huffman tables (ntab <= RART_JPEG_MAX_TABLES, RART_JPEG_HUFF_PITCH bytes each, a device-ready
 * image of the decoder's own table) to tabs_host (capacity in bytes; RART_ERR_INVALID when too small).  host_path = 1 marks a file
 * the sequential decoder has to take: a restart interval, a scan of more than RART_JPEG_MAX_SUBSEQ subsequences or 2^19 - 2
 * bytes, more than four distinct tables; its scan_len, nsub and ntab are 0.  What the image needs of the staging buffers:
 * scan_len bytes of `scans` (the file's bytes from scan_pos on) and ntab * RART_JPEG_HUFF_PITCH bytes of `tabs`.
 *
 * rart_jpeg_entropy_decode_gpu: scan / scan_host hold the same n descriptors on the device and on the host.  Host-path images
 * come first and are skipped (status RART_OK, rounds_used 0, their coefficients untouched: the caller put them there); the
 * coefficients of all others are zeroed and written.  block_start numbers an image's first block as rart_jpeg_desc.block_start[0]
 * does, sub_start counts the subsequences of the images before it.  Every offset and size of the host copy is checked against
 * scans_bytes, tabs_bytes, total_blocks and workspace_bytes BEFORE any launch; in the kernel every byte read is checked against
 * the image's scan_len, every store against its block total, every loop is bounded by a count fixed at launch, and no workgroup
 * waits for another.  status / rounds_used: device int32[n].  One memset + one launch.
 *
 * rart_jpeg_entropy_emulate is HOST-ONLY: the same rounds, cap, prefix sums and write pass from the same source on the CPU, for
 * one file (a host-path file goes through the sequential decoder, rounds_used 0).  Statuses as above; coef_host as
 * rart_jpeg_entropy_decode writes it (written for RART_OK / RART_ERR_INVALID only). */
#define RART_JPEG_DEFAULT_SUBSEQ_BYTES 512
#define RART_JPEG_DEFAULT_MAX_ROUNDS 14
#define RART_JPEG_MAX_SUBSEQ 4096
#define RART_JPEG_MAX_TABLES 4
#define RART_JPEG_HUFF_PITCH 1504
typedef struct rart_jpeg_scan {
  int64_t scan_off;               /* caller: byte of `scans` where the image's scan_len bytes start */
  int64_t tab_off;                /* caller: byte of `tabs` where its ntab tables start, a multiple of 16 */
  int64_t block_start;            /* caller: the image's first block in `coef` */
  int64_t sub_start;              /* caller: subsequences of the images before it (indexes the workspace) */
  int64_t scan_pos;               /* plan: byte of the file where the entropy-coded segment starts */
  int32_t scan_len;               /* plan: bytes from scan_pos to the first marker or the end of the file */
  int32_t nsub;                   /* plan: ceil(scan_len / subseq_bytes) */
  int32_t host_path, ntab;
  int32_t dc_tab[3], ac_tab[3];   /* plan: each component's tables, as indices into the image's ntab tables */
  int32_t ncomp, h_samp, v_samp;  /* luma's sampling factors */
  int32_t mcux, mcuy;
  int32_t blocks_w[3], blocks_h[3];
  int32_t reserved_;
} rart_jpeg_scan;
int rart_jpeg_scan_plan(const uint8_t* data_host, size_t len, const rart_jpeg_info* info_host, int subseq_bytes,
                        rart_jpeg_scan* scan_host, void* tabs_host, size_t tabs_capacity);
size_t rart_jpeg_entropy_workspace_bytes(const rart_jpeg_scan* scan_host, int n);
int rart_jpeg_entropy_decode_gpu(const rart_jpeg_scan* scan, const rart_jpeg_scan* scan_host, int n, const uint8_t* scans,
                                 size_t scans_bytes, const uint8_t* tabs, size_t tabs_bytes, int16_t* coef, int64_t total_blocks,
                                 int subseq_bytes, int max_rounds, int32_t* status, int32_t* rounds_used, void* workspace,
                                 size_t workspace_bytes, rart_stream_t stream);
int rart_jpeg_entropy_emulate(const uint8_t* data_host, size_t len, const rart_jpeg_info* info_host, int subseq_bytes,
                              int max_rounds, int16_t* coef_host, size_t capacity, int32_t* rounds_used);

/* ---------------------------------------------------------------------------------------
 * Batched variable-size resize (csrc/resize_batch.hip): Pillow's Image.resize for 8-bit RGB for n images of DIFFERENT sizes in one
 * call -- crop(box), resize to (resize_h, resize_w) with filter 0..5, the crop window (crop_y, crop_x, crop_h, crop_w) of the
 * target, then an optional left-right mirror: what imagenet_s_gen.py:119-120 and torchvision's resized_crop compute.  The box is a
 * hard boundary (the filter support never reads outside it; Image.resize(box=...) does).  Arithmetic: that of rart_pil_resize_u8
 * for the filtered operators.
 * Two launches per call for the filtered operators, one for NEAREST, whatever n and however the sizes mix.
 *
 * rart_resize_batch_plan is HOST-ONLY (no HIP call).  The caller fills src, h, w, box_* and flip of n descriptors; the plan entry
 * writes into plan_host, a buffer of `capacity` bytes, four regions, each 16-byte aligned, behind one another:
 *   rart_resize_plan header    : the call's parameters, the element counts and byte offsets of the regions, and workspace_bytes
 *   n rart_resize_desc         : the caller's fields plus the derived ones
 *   n + 1 int64 prefix         : prefix[i] = first-pass work items (= bytes of the uint8 intermediate) of the images before i;
 *                                image i has mid_count_i * crop_w * 3 of them (vfirst: crop_h * mid_count_i * 3).  NEAREST: all zero.
 *   table_count int32          : the coefficient tables, rows [xmin, count, k0 .. k_{ksize-1}] (22-bit fixed point), each distinct
 *                                (in_size, out_size, filter) of the call stored once however many images share it.  NEAREST: index
 *                                tables instead, out_size entries each = the source column / row of every output column / row,
 *                                from Pillow's double accumulation (Geometry.c ImagingScaleAffine)
 * `sizes` (optional) receives the same header; sizes->total_bytes is the buffer size the call needs = 80 + 64 n +
 * 16-aligned(8 (n + 1)) + 4 table_count.  With plan_host NULL only `sizes` is filled (RART_OK); a capacity below total_bytes is
 * RART_ERR_WORKSPACE and nothing is written.
 * The caller moves plan_host[0 .. total_bytes) to the device in ONE copy (16-byte aligned) and passes both copies to
 * rart_resize_batch_u8, which validates the HOST copy before any launch: the count, the filter, the crop window inside the
 * target, every box inside its image, the region offsets, every table offset and every tap range the kernels will read, the
 * prefix table, workspace_bytes >= header.workspace_bytes and out_bytes >= n crop_h crop_w 3 -- so no descriptor can make a kernel
 * read or write outside the caller's buffers (RART_ERR_INVALID / RART_ERR_WORKSPACE).  out: uint8 [n][crop_h][crop_w][3]. */
typedef struct rart_resize_desc {
  uint64_t src;                           /* device address of the image, uint8 [h][w][3] */
  int32_t h, w;
  int32_t box_y, box_x, box_h, box_w;     /* the source box, inside the image */
  int32_t flip;                           /* non-zero: mirror the output left-right */
  /* derived by rart_resize_batch_plan */
  int32_t mid_first, mid_count;           /* rows (vfirst: columns) of the box, relative to it, that the first pass produces */
  int32_t tab_h, ks_h, tab_v, ks_v;       /* int32 element of the table region where the table starts; its taps per row (NEAREST: 0) */
  int32_t vfirst;                         /* 1: vertical pass first, as PIL's resize() does when box_h > 100 box_w and the height shrinks */
} rart_resize_desc;
typedef struct rart_resize_plan {
  int32_t n, filter, resize_h, resize_w, crop_y, crop_x, crop_h, crop_w;
  int64_t desc_off, prefix_off, table_off;    /* byte offsets from the start of the buffer */
  int64_t table_count;                        /* int32 elements */
  int64_t workspace_bytes, total_bytes;
} rart_resize_plan;
int rart_resize_batch_plan(const rart_resize_desc* images_host, int n, int filter, int resize_h, int resize_w, int crop_y, int crop_x,
                           int crop_h, int crop_w, void* plan_host, size_t capacity, rart_resize_plan* sizes);
int rart_resize_batch_u8(const void* plan, const void* plan_host, size_t plan_bytes, void* workspace, size_t workspace_bytes,
                         uint8_t* out, size_t out_bytes, rart_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Batched variable-size resize, OpenCV family (csrc/resize_cv_batch.hip): cv2.resize for 8-bit 3-channel images for n images of
 * DIFFERENT sizes in one call -- the box of each image, cv2.resize to (resize_w, resize_h) with interpolation 0..4 (INTER_NEAREST,
 * LINEAR, CUBIC, AREA, LANCZOS4), the crop window of the target, then an optional left-right mirror.  Image k of `out` holds the
 * bytes rart_cv_resize_u8 gives for the box of image k alone; the box is a hard boundary (edge taps replicate the box's border,
 * not the image's) and the row stride is the image's width.  The counterpart of the rart_resize_batch_* pair above, with the same
 * shape: a host-only plan entry, one buffer that crosses the bus in one copy, validation of the host copy before any launch.
 * At most two launches per call, whatever n and however the sizes mix; one when no image of the batch takes the two-pass path.
 *
 * cv2.resize chooses its code from the source size and the target, so the PATH is a field of the descriptor, not of the call:
 *   RART_CV_PATH_NEAREST   : gather; tables = the source column / row of every target column / row, min(floor(d * scale), size - 1)
 *   RART_CV_PATH_TWO_PASS  : LINEAR / CUBIC / LANCZOS4, and AREA with an up-scaling axis (area-mode coordinates): horizontal pass
 *                            into an int32 intermediate, vertical pass with OpenCV's fixed-point casts.  Table rows
 *                            [first tap (may lie outside: taps clamp to the box), k0 .. k_{ks-1}], ks = 2, 4 or 8
 *   RART_CV_PATH_AREA_FLOAT: AREA, both scales >= 1, fractional: float accumulation in OpenCV's order.  Table rows
 *                            [count, (source index, alpha as float bits) x ks], ks = the largest count of the table
 *   RART_CV_PATH_AREA_INT  : AREA with integer scales, and LINEAR with an exact 2 x 2 decimation (cv2 executes it as AREA): no
 *                            tables; ks_x / ks_y hold the integer scales, (a+b+c+d+2)>>2 for 2 x 2, rintf(sum * (1.f / area)) otherwise
 *
 * rart_cv_resize_batch_plan is HOST-ONLY (no HIP call).  The caller fills src, h, w, box_* and flip of n descriptors; the plan
 * entry writes into plan_host, a buffer of `capacity` bytes, four regions, each 16-byte aligned, behind one another:
 *   rart_cv_resize_plan header : the call's parameters, the element counts and byte offsets of the regions, and workspace_bytes
 *   n rart_cv_resize_desc      : the caller's fields plus the derived ones
 *   n + 1 int64 prefix         : prefix[i] = int32 samples of the intermediates of the images before i; a two-pass image has
 *                                mid_count_i * crop_w * 3 of them (the rows of its box that the crop window's vertical taps read, the
 *                                crop window's columns), every other image none
 *   table_count int32          : the tables, each distinct (source size, target size, interpolation, axis) of the call stored once
 *                                however many images share it
 * `sizes` (optional) receives the same header; sizes->total_bytes is the buffer size the call needs = 80 + 64 n +
 * 16-aligned(8 (n + 1)) + 4 table_count, and sizes->workspace_bytes = 256-aligned(4 prefix[n]).  With plan_host NULL only `sizes`
 * is filled (RART_OK); a capacity below total_bytes is RART_ERR_WORKSPACE and nothing is written.
 * The caller moves plan_host[0 .. total_bytes) to the device in ONE copy (16-byte aligned) and passes both copies to
 * rart_cv_resize_batch_u8, which validates the HOST copy before any launch: the count, the interpolation, the crop window inside
 * the target, the region offsets, every box inside its image, every path code, every table offset and row inside the table region,
 * every tap and area index the kernels will form (after the clamp they apply) inside the box, the intermediate ranges, the prefix
 * table, plan_bytes, workspace_bytes >= header.workspace_bytes and out_bytes >= n crop_h crop_w 3 -- so no descriptor can make a
 * kernel read or write outside the caller's buffers (RART_ERR_INVALID / RART_ERR_WORKSPACE).  src may be any byte address (the
 * kernels read it byte by byte).  out: uint8 [n][crop_h][crop_w][3]. */
#define RART_CV_PATH_NEAREST 0
#define RART_CV_PATH_TWO_PASS 1
#define RART_CV_PATH_AREA_FLOAT 2
#define RART_CV_PATH_AREA_INT 3
typedef struct rart_cv_resize_desc {
  uint64_t src;                           /* device address of the image, uint8 [h][w][3] */
  int32_t h, w;
  int32_t box_y, box_x, box_h, box_w;     /* the source box, inside the image */
  int32_t flip;                           /* non-zero: mirror the output left-right */
  /* derived by rart_cv_resize_batch_plan */
  int32_t path;                           /* RART_CV_PATH_* */
  int32_t tab_x, ks_x, tab_y, ks_y;       /* int32 element of the table region where the table starts, and ks as the path defines it */
  int32_t mid_first, mid_count;           /* two-pass: rows of the box, relative to it, that the horizontal pass produces; else 0 */
} rart_cv_resize_desc;
typedef struct rart_cv_resize_plan {
  int32_t n, interpolation, resize_h, resize_w, crop_y, crop_x, crop_h, crop_w;
  int64_t desc_off, prefix_off, table_off;    /* byte offsets from the start of the buffer */
  int64_t table_count;                        /* int32 elements */
  int64_t workspace_bytes, total_bytes;
} rart_cv_resize_plan;
int rart_cv_resize_batch_plan(const rart_cv_resize_desc* images_host, int n, int interpolation, int resize_h, int resize_w, int crop_y,
                              int crop_x, int crop_h, int crop_w, void* plan_host, size_t capacity, rart_cv_resize_plan* sizes);
int rart_cv_resize_batch_u8(const void* plan, const void* plan_host, size_t plan_bytes, void* workspace, size_t workspace_bytes,
                            uint8_t* out, size_t out_bytes, rart_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROBUSTART_HIP_H */
