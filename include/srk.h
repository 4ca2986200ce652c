/*
 * srk.h — C ABI of libsrk.so, the MI355X (gfx950 / CDNA4) kernel library behind the
 * convolutional super-resolution hot path.
 *
 * The reference (togheppi/pytorch-super-resolution-model-collection) has no FFI layer: its
 * hot path is the set of torch.nn calls made by base_networks.py and the per-model Net
 * classes.  Each entry point below names the reference call site (file:line under
 * /root/reference) whose arithmetic it replaces.  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 data owned by the caller; the library never
 *     allocates or frees, and does not retain a pointer past the call
 *   - activations are dense NHWC ("channels_last"): x[n][h][w][c];
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*) of the CURRENT
 *     device (hipSetDevice is the caller's job); no call synchronises the device;
 *     -- with ONE sanctioned exception: between srk_wgrad_reduce_defer(1) and the next
 *     srk_wgrad_reduce_flush() the calling thread's weight-gradient calls queue their slab
 *     reductions, and the queue holds their workspace / dw / db pointers until that flush (the
 *     contract is spelled out at srk_wgrad_reduce_defer);
 *   - calls may be made concurrently from several host threads and for several devices of one
 *     process.  The library's mutable state is: thread-local -- the last-error string, the name
 *     of the last dispatched kernel (srk_last_kernel_name, a diagnostic), the deferred-reduction
 *     queue above, and the two deprecated srk_last_conv_* values (results now come back through
 *     the out-fields of srk_epilogue); process-wide -- one atomic "dynamic-LDS limit raised"
 *     flag per (kernel, device) (hipFuncSetAttribute is a per-device property, set on a kernel's
 *     first large-LDS launch on that device), a mutex-guarded cache of LDS layouts per tile
 *     geometry (conv_bfd), the SRK_* debugging environment switches, each read once, and the
 *     device-side timeout counter behind srk_ring_timeouts();
 *   - return value: SRK_OK (0) or a negative srk_status; no exception crosses the ABI.
 */
#ifndef SRK_H_
#define SRK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRK_VERSION 600 /* major*10000 + minor*100 + patch; 0.6.0: srk_conv2d_forward_ex + srk_conv_result, the pair entry points retired */

typedef enum srk_status {
  SRK_OK = 0,
  SRK_ERR_BAD_ARG = -1,     /* null pointer, non-positive dim, inconsistent shapes        */
  SRK_ERR_INVALID = SRK_ERR_BAD_ARG, /* the same status under the name the degradation entry points document */
  SRK_ERR_UNSUPPORTED = -2, /* legal request that no kernel in this build covers          */
  SRK_ERR_LAUNCH = -3,      /* hipGetLastError() != hipSuccess after a launch             */
  SRK_ERR_WORKSPACE = -4    /* caller-provided workspace smaller than srk_*_workspace_bytes */
} srk_status;

/* Activation kinds: base_networks.py:50-60 (ReLU / PReLU / LeakyReLU(0.2) / Tanh / Sigmoid). */
typedef enum srk_act {
  SRK_ACT_NONE = 0,
  SRK_ACT_RELU = 1,
  SRK_ACT_PRELU = 2, /* slope(s) read from device memory (learnable, base_networks.py:54) */
  SRK_ACT_LRELU = 3, /* slope passed by value (0.2 in the reference, base_networks.py:56)  */
  SRK_ACT_TANH = 4,
  SRK_ACT_SIGMOID = 5
} srk_act;

/* Which implementation a conv call may use.  AUTO picks the fastest kernel that covers the
 * shape; GENERIC forces the plain gather kernel (used by the tests to cross-check).  The environment
 * variable SRK_FORCE_ALGO=generic|mfma|direct|bf16x3|bf16x6 overrides AUTO (SRK_FORCE_ALGO=mfma gives the
 * exact-fp32 MFMA path everywhere). */
typedef enum srk_algo {
  SRK_ALGO_AUTO = 0,        /* bf16x3 MFMA where it applies, else fp32 MFMA / direct / generic            */
  SRK_ALGO_GENERIC = 1,     /* plain fp32 gather kernel (any shape)                                       */
  SRK_ALGO_MFMA = 2,        /* exact fp32 MFMA (v_mfma_f32_16x16x4_f32)                                    */
  SRK_ALGO_DIRECT = 3,      /* fp32 VALU kernel for Cout <= 4                                              */
  SRK_ALGO_MFMA_BF16X3 = 4, /* 3-term bf16 split on v_mfma_f32_16x16x32_bf16, fp32 accumulate (~1e-5 rel) */
  SRK_ALGO_MFMA_BF16X6 = 5, /* exact 3-way operand split, 6 bf16 MFMAs per product: fp32-faithful (~1e-7
                               rel) at 2.7x the fp32-MFMA rate; shapes it does not cover run SRK_ALGO_MFMA */
  SRK_ALGO_MFMA_F16X3 = 6   /* fp32-faithful with THREE MFMAs per product: both operands scaled by a power of two (exact)
                               so that their largest magnitude sits at 2^13..2^14, split x = h + m into two fp16 planes
                               (2 x 11 significant bits), products m*h + h*m + h*h on v_mfma_f32_16x16x32_f16, fp32
                               accumulate, exact power-of-two descale (~1.2e-7 rms vs 0.8e-7 for plain fp32).  Needs
                               an upper bound of max|x| on the device (srk_epilogue.x_amax); forward convs the fp16
                               kernels cover (srk_conv2d_f16x3_supported), SRK_ERR_UNSUPPORTED elsewhere */
} srk_algo;

/* A device-side running maximum of |values|: SRK_AMAX_FLOATS floats = SRK_AMAX_SLOTS slots, one per 64-byte line (slot
 * i is float 16 i: atomics on one line serialise in one L2 channel, so the kernels spread theirs over the slots); the
 * value is the maximum over the slots.  Zero the buffer before the first producer; any upper bound is a valid content. */
#define SRK_AMAX_SLOTS 16
#define SRK_AMAX_FLOATS 256

/* Geometry of one torch.nn.Conv2d / ConvTranspose2d call.
 *   conv       (base_networks.py:42,112-113,156): y[n,oy,ox,co] = sum x[n,oy*s-p+kh,ox*s-p+kw,ci] * w
 *   transposed (base_networks.py:77, fsrcnn.py:33):  y[n,oy,ox,co] = sum x[n,(oy+p-kh)/s,(ox+p-kw)/s,ci] * w
 * (H,W,Cin) describe x and (OH,OW,Cout) describe y in both cases; OH/OW must equal
 * srk_conv_out_dim(). */
typedef struct srk_conv_desc {
  int32_t N, H, W, Cin;
  int32_t OH, OW, Cout;
  int32_t KH, KW;
  int32_t stride, pad;
  int32_t transposed; /* 0: Conv2d, 1: ConvTranspose2d */
  int32_t out_pad;    /* ConvTranspose2d output_padding (fsrcnn.py:33 uses 1) */
  int32_t algo;       /* srk_algo */
  int32_t x_nchw;     /* forward only: x is the caller's NCHW tensor (read in place by the Cin <= 4 bf16x3
                         first-layer kernel; SRK_ERR_UNSUPPORTED elsewhere) */
  int32_t dy_ps_r;    /* backward only: dy is handed over in the pixel-shuffled layout [N, OH*r, OW*r, Cout/r^2] that the
                         fused conv + PixelShuffle forward produced (PSBlock, base_networks.py:179-181); the bf16x3
                         data- and weight-gradient kernels un-shuffle while staging (SRK_ERR_UNSUPPORTED elsewhere:
                         call srk_pixel_shuffle_backward first) */
} srk_conv_desc;

/* Fused epilogue of a forward conv:  y = PS_r( act(conv + bias) ) + residual
 *   bias     : Conv2d bias (may be NULL — vdsr.py:17-24 and lapsrn.py are bias-free)
 *   act      : ConvBlock activation (base_networks.py:67-70)
 *   residual : torch.add(out, residual) of ResnetBlock / VDSR / EDSR / SRGAN
 *              (base_networks.py:149, vdsr.py:31, edsr.py:42, srgan.py:39); indexed like y
 *   ps_r     : PSBlock's PixelShuffle(r) fused into the store (base_networks.py:157,179-181);
 *              0 or 1 = none.  With ps_r>1, y is [N, OH*r, OW*r, Cout/r^2]. */
typedef struct srk_epilogue {
  const float* bias;
  const float* prelu_weight; /* SRK_ACT_PRELU: device slopes */
  const float* residual;
  float slope;               /* SRK_ACT_LRELU */
  int32_t act;               /* srk_act */
  int32_t prelu_n;           /* 1 (nn.PReLU() default) or number of output channels */
  int32_t ps_r;
  const float* x_amax;       /* SRK_ALGO_MFMA_F16X3: SRK_AMAX_FLOATS floats, max over the slots >= max|x| (NULL otherwise) */
  float* y_amax;             /* optional: SRK_AMAX_FLOATS floats that receive (atomic max) max|y| of this call's output
                                -- the next layer's x_amax.  Honoured by the kernels listed at srk_conv2d_f16x3_supported;
                                srk_conv2d_forward_ex reports whether the dispatched kernel did (srk_conv_result) */
  double* bn_partial;        /* optional (forward): the conv leaves the per-channel column sums of its OUTPUT for the
                                BatchNorm behind it (base_networks.py:46,117: conv -> bn) -- row t of
                                [tiles][2 * Cout] doubles = {sum y, sum y*y} over the pixels of tile t, summed in a fixed
                                order; room for N * ceil(OH / 8) * ceil(OW / 8) rows.  Honoured by the per-tile 64 -> 64
                                3x3 kernel (k_c64) only: srk_conv_result.bn_partial_rows says how many rows the call wrote
                                (0: none -- run srk_bn_stats_finalize as usual), srk_bn_finalize_partials() consumes them */
} srk_epilogue;  /* (layout frozen at library version 600 = the round-4 layout: results of a call travel in srk_conv_result, never here) */

/* What the kernel a forward call dispatched to did -- a HOST struct the caller owns, filled by srk_conv2d_forward_ex.
 * `struct_size` is set by the CALLER to sizeof(srk_conv_result) of the header it was compiled against: the library writes
 * only the fields that fit, so the struct can grow without breaking older callers. */
typedef struct srk_conv_result {
  uint32_t struct_size;
  int32_t wrote_amax;       /* 1: the kernel keeps the running maximum of |y| in ep->y_amax (and y_amax was given) -- only
                               then may the slots be handed to the next layer as x_amax (base_networks.py:101-104) */
  int32_t bn_partial_rows;  /* rows of ep->bn_partial the call filled (0: none -- run srk_bn_stats_finalize as usual) */
} srk_conv_result;

/* Activation-gradient prologue of the backward kernels: the incoming gradient dy is
 * multiplied by act'(.) while it is loaded, using the SAVED FORWARD OUTPUT `y`
 * (post-activation; valid for ReLU and positive-slope LeakyReLU, which is what
 * ReLU(True)/LeakyReLU(0.2, True) in base_networks.py:52,56 keep alive). */
typedef struct srk_bwd_mask {
  const float* y; /* NULL = no mask */
  float slope;    /* 0 for ReLU */
} srk_bwd_mask;

/* ---- queries --------------------------------------------------------------------------- */
int srk_version(void);
const char* srk_status_string(int status);
const char* srk_last_error_string(void); /* thread-local, valid until the next failing call */
/* Name (with template arguments) of the kernel the calling thread's last srk_conv2d_forward / _backward_data call
 * dispatched to, e.g. "k_conv_bfw<2,9,2>" — what a measurement should quote (thread-local, never NULL). */
const char* srk_last_kernel_name(void);
/* DEPRECATED aliases of srk_conv_result.wrote_amax / .bn_partial_rows (thread-local side channels that have to be queried
 * before the thread's next conv call; kept for callers written against the round-4 header). */
int srk_last_conv_wrote_amax(void);
int srk_last_conv_bn_partial_rows(void);
/* Diagnostic of the ring kernels (k_conv_bfr: producer and consumer waves of a persistent block hand halo buffers over
 * through counters in LDS, every poll has an iteration cap): number of polls that ran into the cap since the last
 * reset (k_espcn_pair's included) -- 0 in a correct library.  Synchronises the device; tests and fuzzers call it, the product never does. */
int srk_ring_timeouts(int reset);
/* Output spatial size of a conv / transposed conv along one axis (torch semantics). */
int srk_conv_out_dim(int in, int k, int stride, int pad, int transposed, int out_pad);

/* ---- host planners, as diagnostics ------------------------------------------------------- */
/* What the library's host planners decide, for tests and measurements: no device, no stream, no allocation, nothing is
 * launched.  Every out-struct is a HOST struct sized by the caller through a leading struct_size, as srk_conv_result is.
 * (Added without a change of srk_version(): new entry points only, nothing existing changed.) */
enum { SRK_WGRAD_KERNEL_BF = 0, SRK_WGRAD_KERNEL_TR = 1 }; /* k_wgrad_bf | k_wgrad_tr */
/* The launch the stride-1 bf16x3 weight gradient makes of a problem, when srk_conv2d_backward_weight[_grouped] hands it one
 * (SRK_ALGO_AUTO / _MFMA_BF16X3, not a few-output-channel layer). */
typedef struct srk_wgrad_plan {
  uint32_t struct_size;
  int32_t ok;                    /* 0: these kernels do not cover the problem (every other field is 0) */
  int32_t kernel;                /* SRK_WGRAD_KERNEL_* */
  int32_t cfg, CIB, COB;         /* tile configuration 0..2: input x output channels of a block */
  int32_t spec, k33;             /* wave-specialised variant (else one tile per block step); its 3x3 K loop */
  int32_t prefetch, ring;        /* spec: the stagers load one tile ahead; X halo rows live in a ring */
  int32_t vec_x, vec_y, scalar;  /* 16-byte loads of x / of dy and the mask (channels a multiple of 4, pointers on 16-byte
                                    boundaries); scalar = not both: what the name says, and no prefetch */
  int32_t grouped, n;            /* the grouped entry, its layers (per-layer entry: 0, 1) */
  int32_t G;                     /* split-K partial slabs per layer */
  int32_t grid_x, grid_y, grid_z, block, lds_bytes; /* the launch: blocks, threads, dynamic LDS */
  int32_t TH, TW, TWo, HH, HWp, CS, DS, nks;        /* tile rows / pixels / octets per row, halo rows / padded width, plane strides, K steps */
  int32_t tiles_y, tiles_x, ntiles, gy, gz;         /* tiles per image and in all; input / output channel chunks */
  int32_t lds_set, ring_bytes;   /* LDS of one buffer set; of the ring layout (0 without it) */
  int32_t XP, XPL, YPL;          /* k_wgrad_tr: pixels per ring row, bytes per X / dY plane */
  uint64_t slab_bytes, ws_bytes; /* workspace: the partial slabs in front of the bias partials; all of it */
  char name[64];                 /* what srk_last_kernel_name() reports after the launch */
} srk_wgrad_plan;
/* n_layers = 1: srk_conv2d_backward_weight; > 1: one grouped launch of that many layers.  x_aligned / dy_aligned: x / dy
 * and the mask are on 16-byte boundaries.  num_cu: compute units to plan for, 0 = the current device's.  out->struct_size
 * must be set.  SRK_OK also when the plan says ok = 0. */
int srk_conv2d_backward_weight_plan(const srk_conv_desc* d, int n_layers, int x_aligned, int dy_aligned, int num_cu,
                                    srk_wgrad_plan* out);
/* The stride-1 problems a strided TRANS gather (ConvTranspose2d forward, data gradient of a strided Conv2d) is split into,
 * one per output phase.  One axis: the phase writes outputs o0 + r * stride, r < P; its virtual tap u reads input
 * r + i0 + u and weight tap w0 + wd * u, u < Kv (Kv = 0: no tap reaches the phase, i0 = w0 = wd = 0). */
typedef struct srk_phase_axis {
  uint32_t struct_size;
  int32_t o0, P, Kv, i0, w0, wd;
} srk_phase_axis;
/* Both axes; a phase without taps on either axis has none at all (KHv = KWv = 0 and zero tap fields). */
typedef struct srk_phase {
  uint32_t struct_size;
  int32_t oy0, ox0, PH, PW, KHv, KWv, iy0, ix0, wh0, wdh, ww0, wdw;
} srk_phase;
/* Fill out[0 .. count) with the phases that run (a phase whose first output lies outside O does not), in launch order,
 * and return count.  out[0].struct_size must be set: it is the size and stride of the caller's elements.  Negative
 * srk_status on bad arguments or when max is too small. */
int srk_trans_phase_axis(int K, int stride, int pad, int O, srk_phase_axis* out, int max);
int srk_trans_phases(int KH, int KW, int stride, int pad, int OH, int OW, srk_phase* out, int max);

/* ---- layout ---------------------------------------------------------------------------- */
/* NCHW <-> NHWC copies at the module boundary (the reference feeds NCHW tensors:
 * edsr.py:146-152). */
int srk_nchw_to_nhwc(const float* x, float* y, int N, int C, int H, int W, void* stream);
int srk_nhwc_to_nchw(const float* x, float* y, int N, int C, int H, int W, void* stream);

/* Weight repacks.  `w` is the state_dict tensor exactly as torch stores it:
 *   Conv2d          [Cout][Cin][KH][KW]   (transposed = 0)
 *   ConvTranspose2d [Cin][Cout][KH][KW]   (transposed = 1)
 * Packed layout consumed by srk_conv2d_forward:        wp[kh][kw][ci][co]
 * Packed layout consumed by srk_conv2d_backward_data:  wp[kh][kw][co][ci]
 *   (for the data gradient the roles of the channel axes swap; the spatial flip is handled by
 *   the kernels' index arithmetic, not by the packing).
 * ps_r > 1 (forward only) additionally permutes the output channels to (i, j, c) order so a
 * fused pixel-shuffle store is contiguous; bias must then be packed with srk_pack_bias_ps.
 * A packed buffer is srk_packed_weight_bytes() long: the fp32 layout above followed (256-byte
 * aligned) by the same filter pre-split into bf16 hi/lo planes for the bf16x3 MFMA kernel. */
size_t srk_packed_weight_bytes(int Cout, int Cin, int KH, int KW, int bwd);
int srk_pack_weight_fwd(const float* w, float* wp, int Cout, int Cin, int KH, int KW, int transposed, int ps_r,
                        void* stream);
/* bwd, ps_r > 1: the contraction axis (Cout) is ordered (i, j, c) — the channel order of a pixel-shuffled dy, for
 * srk_conv2d_backward_data with srk_conv_desc.dy_ps_r set */
int srk_pack_weight_bwd(const float* w, float* wp, int Cout, int Cin, int KH, int KW, int transposed, int ps_r,
                        void* stream);
int srk_pack_bias_ps(const float* b, float* bp, int Cout, int ps_r, void* stream);
/* Whole-model packing (training: the weights change every step).  `params_base` is the flat fp32 parameter buffer,
 * `packed_base` a caller-owned byte buffer, `table` a DEVICE array of n_layers rows x 14 int64:
 *   0 w_off (floats)  1 fwd_off (bytes, -1 skip)  2 bwd_off (bytes, -1 skip)  3 Cout  4 Cin  5 KH  6 KW  7 transposed
 *   8 ps_r  9 bias_off (floats, -1)  10 bias_ps_off (bytes, -1)
 *   11 amax_off (bytes into packed_base, -1 none): a 4-byte scratch word per layer, ZEROED BY THE CALLER before the call,
 *      that lets the layer's max|w| (scale of the fp16 planes of SRK_ALGO_MFMA_F16X3) be taken by parallel slices
 *      instead of one block per layer; pass -blocks_per_layer when every row has one (skips the single-block pass)
 *   12 first block of the layer in `fast_blocks` (-1: generic path)  13 reserved (0)
 * Every fwd_off / bwd_off region receives exactly what srk_pack_weight_fwd / _bwd would write there.
 * fast_blocks (DEVICE, may be NULL): n_fast_blocks pairs {layer, local block} for the layers with column 12 >= 0 -- plain
 * Conv2d filters (not transposed, KH*KW <= 25, Cout = 32 or a multiple of 64, Cin = 16 / 32 / 48 or a multiple of 64 --
 * no channel padding in any prepared layout --, both directions wanted) take
 * (Cout / 8) * ceil(Cin / 32) blocks each, local block = octet * ceil(Cin / 32) + chunk; a block reads its 8 x 32-channel
 * filter tile once, coalesced, and writes all layouts from LDS (the generic path gathers every value separately). */
int srk_pack_weights_batched(const float* params_base, void* packed_base, const int64_t* table, int n_layers,
                             int blocks_per_layer, const int32_t* fast_blocks, int n_fast_blocks, void* stream);
/* max|x| over n floats into an SRK_AMAX_FLOATS buffer (atomic max: zero it first) -- x_amax of a tensor no kernel
 * of this library produced (the network input). */
int srk_absmax(const float* x, size_t n, float* amax_slots, void* stream);
/* 1 when srk_conv2d_forward(d, ..., ep) with d->algo = SRK_ALGO_MFMA_F16X3 has a kernel: Conv2d / ConvTranspose2d with
 * Cin >= 8, Cout >= 8, and first layers (Cin <= 4 Conv2d, Cout a multiple of 16, also with x_nchw), every output group
 * on the 16-byte store path.  Those kernels (k_conv_bfd, k_conv_bfw, k_conv_bf3_rows) also fill ep->y_amax -- in every
 * arithmetic they run, not only f16x3; so do k_c64, the exact-fp32 MFMA kernels and the 4-wave vector form of k_conv_bf3
 * (stride-1 and Conv2d gathers) while every output group is on the 16-byte path.  srk_conv_result.wrote_amax is the
 * authority: where it is 0 the slots are left as they were. */
int srk_conv2d_f16x3_supported(const srk_conv_desc* d, const srk_epilogue* ep, const float* y);

/* ---- convolution (Conv2d / ConvTranspose2d: base_networks.py:42,77,112-113,156; fsrcnn.py:33) */
int srk_conv2d_forward(const srk_conv_desc* d, const float* x, const float* w_packed_fwd, float* y,
                       const srk_epilogue* ep, void* stream);
/* The same call, reporting what the dispatched kernel did in *res (may be NULL = srk_conv2d_forward).  Replaces the
 * thread-local srk_last_conv_* side channels below. */
int srk_conv2d_forward_ex(const srk_conv_desc* d, const float* x, const float* w_packed_fwd, float* y,
                          const srk_epilogue* ep, srk_conv_result* res, void* stream);
/* dx = d(loss)/dx given dy; optional act-grad prologue on dy; optional fused "+ add_to"
 * (gradient fan-in of a residual connection).  Replaces aten::convolution_backward (input
 * gradient) as dispatched from loss.backward() — edsr.py:154, vdsr.py:146, srgan.py:286,309. */
int srk_conv2d_backward_data(const srk_conv_desc* d, const float* dy, const float* w_packed_bwd, float* dx,
                             const srk_bwd_mask* mask, const float* add_to, void* stream);
/* The same gradient, already multiplied by the ReLU gradient of the layer that PRODUCED x (`x_relu` = this conv's
 * input x, the output of an upstream conv + ReLU: dx <- dx * (x_relu > 0)).  The upstream layer's backward
 * (aten::threshold_backward inside loss.backward(), vdsr.py:146) would apply exactly this mask to its dy -- reading x
 * once more in its data-gradient AND its weight-gradient kernel; applied here it costs one read at the output tile,
 * and that layer's srk_conv2d_backward_* calls take mask = NULL.  Only where the wave-specialised kernel runs the
 * gradient (srk_conv2d_backward_data_relu_supported: stride-1 3x3 Conv2d, Cout <= 64 ... of benchmark size);
 * SRK_ERR_UNSUPPORTED otherwise. */
int srk_conv2d_backward_data_relu_supported(const srk_conv_desc* d, const float* dy, const float* dx, const srk_bwd_mask* mask);
int srk_conv2d_backward_data_relu(const srk_conv_desc* d, const float* dy, const float* w_packed_bwd, float* dx,
                                  const srk_bwd_mask* mask, const float* x_relu, void* stream);
/* dw (torch layout, see srk_pack_weight_*) and db (may be NULL).  beta = 0 overwrites,
 * beta = 1 accumulates into dw/db (shared weights: lapsrn.py:40,44).  `workspace` holds the
 * split-K partial sums; size from srk_conv2d_backward_weight_workspace_bytes. */
size_t srk_conv2d_backward_weight_workspace_bytes(const srk_conv_desc* d);
int srk_conv2d_backward_weight(const srk_conv_desc* d, const float* x, const float* dy, const srk_bwd_mask* mask,
                               float* dw, float* db, float beta, void* workspace, size_t workspace_bytes,
                               void* stream);

/* The weight gradients of n convolutions that share ONE geometry `d` — the 32 + 1 body convs of EDSR (edsr.py:37-45),
 * the 18 of VDSR (vdsr.py:17-24), the 32 of SRResNet — in one launch plus one reduce launch.  x / dy / dw / db are HOST
 * arrays of n device pointers (db may be NULL, or hold n non-NULL pointers: bias and bias-free layers cannot share a
 * group), masks a host array of n srk_bwd_mask (NULL = none; an entry's y may be NULL).  No two layers may share a dw
 * (LapSRN's aliased branches go into separate calls).  Same results as n srk_conv2d_backward_weight calls; geometries
 * without a grouped kernel run exactly those.  Nothing but the pointer VALUES is read from the host arrays, at call
 * time (the call is hipGraph-capturable). */
size_t srk_conv2d_backward_weight_grouped_workspace_bytes(const srk_conv_desc* d, int n);
int srk_conv2d_backward_weight_grouped(const srk_conv_desc* d, int n, const float* const* x, const float* const* dy,
                                       const srk_bwd_mask* masks, float* const* dw, float* const* db, float beta,
                                       void* workspace, size_t workspace_bytes, void* stream);
/* Deferred slab reductions.  Every weight-gradient call above ends in a short launch that sums its split-K partial slabs
 * into dw / db.  After srk_wgrad_reduce_defer(1) the calls of this thread queue that reduction instead, and
 * srk_wgrad_reduce_flush(stream) runs everything queued as ONE launch (each reduction in its own summation order: same
 * results bit for bit) -- the end of loss.backward() (edsr.py:154, srgan.py:286,309) is a handful to dozens of such calls.
 * Contract while deferring: every call gets its OWN workspace, alive and untouched until the flush, all calls and the
 * flush use one stream; a second update of a queued dw / db flushes first.  srk_wgrad_reduce_defer returns the previous
 * setting; switching it off does not flush. */
int srk_wgrad_reduce_defer(int on);
int srk_wgrad_reduce_flush(void* stream);

/* ---- residual block, both convolutions in one launch (base_networks.py:109-150 with norm=None, activation='relu':
 * edsr.py:37-45 builds its body from it) ------------------------------------------------------------------------------
 * Forward:   y_mid = relu(conv1(x) + b1),  y = conv2(y_mid) + b2 + x      (3x3, stride 1, pad 1, C -> C -> C)
 * Backward:  d_mid = conv2^T(dy) * (y_mid > 0),  dx = conv1^T(d_mid) + dy
 * Same numbers as the two srk_conv2d_forward / srk_conv2d_backward_data calls they replace (same operand splits,
 * same products; the K-split partial sums meet in a different order).  Only for small problems (strong-scaled shards:
 * srk_resblock2_supported says when): one 8x8 tile per workgroup, the intermediate stays in LDS, and nothing waits for
 * the store -> load round trip between the two convs.  y_mid / d_mid are still written: the weight gradients
 * (srk_conv2d_backward_weight with x = y_mid, dy = dy for conv2 and x = x, dy = d_mid, NO mask, for conv1) need them.
 * algo: SRK_ALGO_MFMA_BF16X6 / SRK_ALGO_MFMA_F16X3 (fp32-faithful; the latter forward only, with x_amax = the
 * SRK_AMAX_FLOATS running-maximum buffer of |x|) or SRK_ALGO_AUTO / SRK_ALGO_MFMA_BF16X3.  y_amax (optional, any algo) receives
 * max|y|.  b1 / b2 may be NULL.
 * Filters: the packed buffers of srk_pack_weight_fwd / srk_pack_weight_bwd (ps_r = 0). */
int srk_resblock2_supported(int N, int H, int W, int C);
int srk_resblock2_forward(int N, int H, int W, int C, const float* x, const float* w1_packed_fwd, const float* b1,
                          const float* w2_packed_fwd, const float* b2, float* y_mid, float* y, int algo,
                          const float* x_amax, float* y_amax, void* stream);
int srk_resblock2_backward_data(int N, int H, int W, int C, const float* dy, const float* w2_packed_bwd,
                                const float* w1_packed_bwd, const float* y_mid, float* d_mid, float* dx, int algo,
                                void* stream);

/* ---- ESPCN's first two convs in one launch (conv_pair.hip) ------------------------------------------------------- */
/* y = relu(conv3x3(relu(conv5x5(x) + b1)) + b2), both "valid", stride 1, f16x3 arithmetic (SRK_ALGO_MFMA_F16X3), inference
 * only; the 64-channel intermediate never leaves the chip.  x: NCHW [N,3,H,W] fp32 (read in place); w1_prepared: what
 * srk_espcn_pair_prepare made of the plain [64,3,5,5] filter and its bias (srk_espcn_pair_prepared_bytes() bytes, 16-byte
 * aligned; once per filter: fragment-ordered fp16 planes, sum |w_c|, |b_c|, max |w|); w2_packed_fwd: srk_pack_weight_fwd of
 * the [32,64,3,3] filter (ps_r = 0); b1 [64], b2 [32]; y: NHWC [N,H-6,W-6,32]; y_amax (optional) receives max|y|.
 * x_amax: the SRK_AMAX_FLOATS running-maximum buffer of |x|.  x_amax_compute == 0: it holds the maximum (or a bound) and
 * is only read.  x_amax_compute != 0: it is ZEROED memory that nothing else uses during the launch; the kernel measures
 * max|x| itself (every block a slice, one rendezvous behind the prologue) and leaves it in the slots, whose words 1 and 2
 * it uses as counters and returns to zero, so a captured launch can be replayed on the same buffer (the slots then hold
 * the running maximum over the replays: never too low).  The output is the same bits as with srk_absmax in front.
 * SRK_ERR_UNSUPPORTED when the shape is not worth the fused kernel (tiles too ragged, fewer than four 8 x 16 tiles per
 * CU) -- the caller runs the two convs then.  force: bit 0 skips that efficiency rule; bit 1 (with x_amax_compute) makes
 * every block take the rendezvous' timeout path, a scan of all of x (tests).
 * srk_espcn_pair_scans: blocks that took that scan path since the last reset (0 in a product run on an idle device; a
 * diagnostic like srk_ring_timeouts, which it is not part of).  Synchronises the device. */
size_t srk_espcn_pair_prepared_bytes(void);
int srk_espcn_pair_prepare(const float* w1, const float* b1, void* w1_prepared, void* stream);
int srk_espcn_pair_forward(int N, int H, int W, const float* x, const void* w1_prepared, const float* b1,
                           const float* w2_packed_fwd, const float* b2, float* y, float* x_amax, int x_amax_compute,
                           float* y_amax, int force, void* stream);
int srk_espcn_pair_scans(int reset);

/* ---- pixel shuffle (torch.nn.PixelShuffle: base_networks.py:157,179-181) ----------------- */
/* x [N,H,W,C*r*r] -> y [N,H*r,W*r,C];  channel c*r*r + i*r + j -> (c, h*r+i, w*r+j). */
int srk_pixel_shuffle_forward(const float* x, float* y, int N, int H, int W, int C, int r, void* stream);
/* dy [N,H*r,W*r,C] -> dx [N,H,W,C*r*r]  (aten::pixel_unshuffle in backward). */
int srk_pixel_shuffle_backward(const float* dy, float* dx, int N, int H, int W, int C, int r, void* stream);

/* ---- pointwise (base_networks.py:50-60,149; vdsr.py:31; edsr.py:42) ------------------------ */
/* y = act(x); channels = innermost (NHWC) extent, used only by per-channel PReLU. */
int srk_act_forward(const float* x, float* y, size_t n, int channels, int act, float slope,
                    const float* prelu_weight, int prelu_n, void* stream);
/* dx = dy * act'(.).  `saved` is the forward INPUT x for PReLU and the forward OUTPUT y for
 * every other kind.  PReLU also accumulates d(slope) into dprelu (+=, caller zeroes). */
int srk_act_backward(const float* dy, const float* saved, float* dx, size_t n, int channels, int act, float slope,
                     const float* prelu_weight, int prelu_n, float* dprelu, void* stream);
/* out = alpha*a + beta*b  (torch.add and autograd's gradient fan-in) */
int srk_axpby(const float* a, const float* b, float* out, size_t n, float alpha, float beta, void* stream);
/* out = x * (*alpha_dev): chain-rule scaling by an upstream scalar gradient that lives on the device
 * (e.g. the 1e-3 weight of the adversarial term, srgan.py:308). */
int srk_scale_dev(const float* x, const float* alpha_dev, float* out, size_t n, void* stream);

/* ---- losses, reduction='mean' (srcnn.py:84-86,129; edsr.py:98-100,153; lapsrn.py:75-85;
 *      srgan.py:157,276-297).  One pass: *loss = mean(...), dpred = d(loss)/d(pred)*grad_scale.
 * pred/dpred are NHWC-dense; target is addressed through explicit element strides
 * (n,c,h,w) so an NCHW target batch needs no copy.  dpred may be NULL (evaluation).
 * `partials` is a caller-provided scratch of srk_loss_workspace_bytes(). */
typedef enum srk_loss { SRK_LOSS_MSE = 0, SRK_LOSS_L1 = 1, SRK_LOSS_CHARBONNIER = 2, SRK_LOSS_BCE = 3 } srk_loss;
size_t srk_loss_workspace_bytes(void);
int srk_loss_forward_backward(int kind, const float* pred, const float* target, const int64_t* target_strides,
                              int N, int C, int H, int W, float eps, float grad_scale, float* loss, float* dpred,
                              void* workspace, void* stream);

/* ---- DRCN recursive-supervision head (drcn.py:38-52, 200-215) ---------------------------------
 * Y = the D reconstructions stacked along the batch axis ([D*N, C, H, W], Y_d = the d-th block of N*C*H*W
 * elements); Y, x, target, out and dY share one dense layout (NHWC in this package; any, as long as it is the same).
 * w = the D combine weights (device).  Sum w is computed on the device: nothing syncs with the host. */
#define SRK_DRCN_MAX_D 32
/* out = x + (sum_d w_d * Y_d) * (1 / sum_d w_d)   (the inference forward) */
int srk_drcn_head_forward(const float* Y, const float* x, const float* w, int D, int N, int C, int H, int W,
                          float* out, void* stream);
/* The training head in one pass over (Y, x, target) plus a one-block finalize (deterministic: no float atomics):
 *   out, *loss = a*mean_d MSE(Y_d, t) + (1-a)*MSE(out, t) + *reg_dev, terms = {mean_d MSE(Y_d, t), MSE(out, t)}
 *   dY_d = s*(a*2(Y_d - t)/(D*M) + g_out*w_d/sum w),  g_out = (1-a)*2(out - t)/M,  M = N*C*H*W, s = grad_scale
 *   dw_d = dw_beta*dw_d + s * sum_pixels g_out*(Y_d - (out - x)) / sum w
 * a = *alpha_dev and the regularisation value *reg_dev (NULL: 0) are read on the device, so a captured hipGraph
 * stays valid when they change.  terms and dw may be NULL.  `workspace`: srk_drcn_workspace_bytes(D). */
size_t srk_drcn_workspace_bytes(int D);
int srk_drcn_head_loss(const float* Y, const float* x, const float* target, const float* w, int D, int N, int C, int H,
                       int W, const float* alpha_dev, const float* reg_dev, float grad_scale, float* out, float* dY,
                       float* loss, float* terms, float* dw, float dw_beta, void* workspace, size_t workspace_bytes,
                       void* stream);
/* Backward of srk_drcn_head_forward for an upstream gradient `dout` of out (same layout as out):
 *   dY_d = dout * w_d / sum w,  dw_d = dw_beta*dw_d + sum_pixels dout*(Y_d - c) / sum w,  c = out - x
 * (c is recomputed from Y and w; dw may be NULL).  `workspace`: srk_drcn_workspace_bytes(D). */
int srk_drcn_head_backward(const float* Y, const float* w, const float* dout, int D, int N, int C, int H, int W,
                           float* dY, float* dw, float dw_beta, void* workspace, size_t workspace_bytes, void* stream);
/* *out = scale * sum_i p_i^2, accumulated in fp64 (drcn.py:212-214: the weight-decay term over a flat parameter
 * buffer).  `workspace`: srk_sumsq_workspace_bytes(). */
size_t srk_sumsq_workspace_bytes(void);
int srk_sumsq(const float* p, size_t n, float scale, float* out, void* workspace, void* stream);

/* ---- optimizers over flat fp32 buffers (srcnn.py:79; fsrcnn.py:105-106; vdsr.py:86-90,149;
 *      espcn.py:79; edsr.py:93; srgan.py:147-149) --------------------------------------------- */
/* torch.optim.SGD: g += wd*p; buf = mom*buf + g (first step: buf = g); p -= lr*(nesterov ? g+mom*buf : buf).
 * `first_step` selects the buf = g initialisation. lr/scale are read from device memory when the
 * *_dev pointers are non-NULL (keeps a captured hipGraph valid across LR decay / grad clipping). */
int srk_sgd_step(float* p, const float* g, float* momentum_buf, size_t n, float lr, float momentum,
                 float weight_decay, int nesterov, int first_step, const float* lr_dev, const float* grad_scale_dev,
                 void* stream);
/* torch.optim.Adam (betas, eps, no amsgrad): `step_dev` points at TWO device int32 {step count, 0}: the kernel works
 * with count + 1 (bias correction) and stores it when its last block finishes; the second word is the kernel's
 * arrival ticket and is 0 between launches. */
int srk_adam_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int32_t* step_dev, const float* lr_dev,
                  const float* grad_scale_dev, void* stream);
/* srk_sgd_step / srk_adam_step that also keep an exponential moving average of the parameters (new entry points only:
 * the two above and srk_version() are unchanged).  `ema` is a buffer laid out like `p`; after the parameter update, from
 * the new value in registers (p is not read again): ema = ema + (1 - ema_decay) * (p_new - ema), a subtraction, a
 * multiply and an add in fp32.  p, the optimizer's buffers and step_dev come out bit-equal to the plain entry point's.
 * The 16-byte form needs `ema` on a 16-byte boundary like the other buffers.  SRK_REQUIRE errors: ema == NULL,
 * ema_decay outside [0, 1) (NaN included). */
int srk_sgd_step_ema(float* p, const float* g, float* momentum_buf, size_t n, float lr, float momentum,
                     float weight_decay, int nesterov, int first_step, const float* lr_dev,
                     const float* grad_scale_dev, float* ema, float ema_decay, void* stream);
int srk_adam_step_ema(float* p, const float* g, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1,
                      float beta2, float eps, float weight_decay, int32_t* step_dev, const float* lr_dev,
                      const float* grad_scale_dev, float* ema, float ema_decay, void* stream);
/* torch.nn.utils.clip_grad_norm (vdsr.py:149): *norm_out = ||g||_2; *scale_out = min(1, max_norm/(norm+1e-6)). */
size_t srk_grad_norm_workspace_bytes(void);
int srk_grad_norm_clip(const float* g, size_t n, float max_norm, float* norm_out, float* scale_out, void* workspace,
                       void* stream);

/* ---- BatchNorm2d, train/eval (base_networks.py:46,117,161; live in srgan.py only) ---------- */
/* Training forward: batch statistics over (N,H,W) per channel, y = (x-mean)*rstd*gamma+beta,
 * running stats updated with `momentum` (unbiased variance), save_mean/save_rstd kept for
 * backward.  sum/sumsq partials are exposed through `stats` ([2*C] doubles: sum, sumsq) so a
 * data-parallel caller can all-reduce them (SyncBN) between the two phases. */
int srk_bn_stats(const float* x, double* stats, size_t rows, int C, void* workspace, void* stream);
size_t srk_bn_workspace_bytes(int C);
/* num_batches_tracked: the module's int64 counter buffer (device), incremented by one; may be NULL */
int srk_bn_finalize(const double* stats, double count, float* save_mean, float* save_rstd, float* running_mean,
                    float* running_var, float momentum, float eps, int C, int64_t* num_batches_tracked, void* stream);
/* srk_bn_stats + srk_bn_finalize in two launches instead of three (single-GPU / per-shard statistics: no all-reduce
 * between the phases); `stats` still receives the [2*C] sums. */
int srk_bn_stats_finalize(const float* x, double* stats, size_t rows, int C, float* save_mean, float* save_rstd,
                          float* running_mean, float* running_var, float momentum, float eps,
                          int64_t* num_batches_tracked, void* workspace, void* stream);
/* The second launch of srk_bn_stats_finalize alone, on column sums a convolution's epilogue left
 * (srk_epilogue.bn_partial: `splits` rows of [2*C] doubles): mean / rstd / running statistics of base_networks.py:46,117's
 * BatchNorm without the pass over the activation.  `rows` = N*H*W of the activation. */
int srk_bn_finalize_partials(const double* partials, int splits, double* stats, size_t rows, int C, float* save_mean,
                             float* save_rstd, float* running_mean, float* running_var, float momentum, float eps,
                             int64_t* num_batches_tracked, void* stream);
/* y_amax (optional, here and in srk_bn_apply_act): SRK_AMAX_FLOATS floats that receive max|y| -- the x_amax of a
 * following SRK_ALGO_MFMA_F16X3 convolution (16-byte path only: C % 4 == 0, aligned tensors). */
int srk_bn_apply(const float* x, float* y, const float* mean, const float* rstd, const float* gamma,
                 const float* beta, size_t rows, int C, int act, float slope, float* y_amax, void* stream);
int srk_bn_eval_params(const float* running_mean, const float* running_var, float eps, float* mean, float* rstd,
                       int C, void* stream);
/* nn.InstanceNorm1d on the [B, F] output of a Linear (DenseBlock(norm='instance'), base_networks.py:12-13): torch reads the
 * 2-D tensor as one unbatched sample of B channels x F positions, i.e. every ROW is normalised with its own biased
 * statistics (no affine parameters, no running statistics).  mean / rstd: [rows] outputs the backward needs. */
int srk_rownorm_forward(const float* x, float* y, float* mean, float* rstd, int rows, int cols, float eps, void* stream);
int srk_rownorm_backward(const float* dy, const float* x, const float* mean, const float* rstd, float* dx, int rows,
                         int cols, void* stream);
/* Backward: `dstats` [2*C] doubles = (sum dy, sum dy*xhat) (all-reducible for SyncBN);
 * srk_bn_backward_apply writes dx = gamma*rstd*(dy - dstats[c]/count - xhat*dstats[C+c]/count)
 * (pass zeros for eval-mode BN); srk_bn_param_grads accumulates dbeta += dstats[c],
 * dgamma += dstats[C+c]. */
int srk_bn_backward_stats(const float* dy, const float* x, const float* mean, const float* rstd, double* dstats,
                          size_t rows, int C, void* workspace, void* stream);
/* srk_bn_backward_stats + srk_bn_param_grads (from the LOCAL sums, as the data-parallel gradient exchange expects) in
 * two launches instead of three; dgamma / dbeta may be NULL. */
int srk_bn_backward_stats_grads(const float* dy, const float* x, const float* mean, const float* rstd, double* dstats,
                                size_t rows, int C, float* dgamma, float* dbeta, void* workspace, void* stream);
int srk_bn_backward_apply(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                          const double* dstats, double count, float* dx, size_t rows, int C, void* stream);
int srk_bn_param_grads(const double* dstats, float* dgamma, float* dbeta, int C, void* stream);
/* BatchNorm with the activation that follows it in the reference's blocks, and the residual add of the BatchNorm
 * ResnetBlock, folded in: act(bn(.)) of ConvBlock / DeconvBlock / PSBlock / DenseBlock (base_networks.py:58-71) and
 * bn(conv2(.)) + x (base_networks.py:141-150).
 *   srk_bn_apply_act:   y = act(gamma * (x - mean) * rstd + beta) [+ residual]   act: NONE / RELU / LRELU / PRELU
 *   srk_bn_backward_stats_grads_act:  dz = dy * act'(z) with z RECOMPUTED from x (nothing of the activation is saved);
 *       dstats = (sum dz, sum dz * xhat), dbeta += / dgamma += those, dprelu += sum_{z <= 0} dy * z (PRELU; NULL ok)
 *   srk_bn_backward_apply_act:        dx = gamma * rstd * (dz - dstats[c]/count - xhat * dstats[C+c]/count)
 * The gradient of `residual` is dy itself.  C must be a multiple of 4, tensors 16-byte aligned.  prelu_n: 1 or C. */
int srk_bn_apply_act(const float* x, float* y, const float* mean, const float* rstd, const float* gamma,
                     const float* beta, size_t rows, int C, int act, float slope, const float* prelu_weight, int prelu_n,
                     const float* residual, float* y_amax, void* stream);
int srk_bn_backward_stats_grads_act(const float* dy, const float* x, const float* mean, const float* rstd,
                                    const float* gamma, const float* beta, double* dstats, size_t rows, int C,
                                    float* dgamma, float* dbeta, int act, float slope, const float* prelu_weight,
                                    int prelu_n, float* dprelu, void* workspace, void* stream);
int srk_bn_backward_apply_act(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                              const float* beta, const double* dstats, double count, float* dx, size_t rows, int C,
                              int act, float slope, const float* prelu_weight, int prelu_n, void* stream);

/* Round 6, "finalize-in-apply": the same BatchNorm in ONE launch less per direction.  The apply kernels finish the split
 * reduction themselves (every block re-sums the partials of its own 16-channel slab in the reduce kernel's order: forward
 * statistics are bit-equal to the calls above), so a training BatchNorm is
 *   forward : [srk_bn_stats_partials |  a conv that left srk_epilogue.bn_partial]  ->  srk_bn_finalize_apply_act
 *   backward:  srk_bn_backward_partials_act                                         ->  srk_bn_backward_finalize_apply_act
 * Per-shard statistics only (SyncBN all-reduces the [2C] sums between the phases: use the calls above).
 * srk_bn_fused_supported(C): C % 16 == 0 and C <= 512.  `partials`: [splits][2][C] doubles (backward with an activation:
 * [splits][3][C]) in a workspace of srk_bn_workspace_bytes(C); *splits_out is a HOST int the partials call fills.
 * What the separate calls return is still returned: stats / dstats [2C], save_mean / save_rstd, running statistics,
 * num_batches_tracked, dgamma += / dbeta += / dprelu +=.  Tensors 16-byte aligned. */
int srk_bn_fused_supported(int C);
int srk_bn_stats_partials(const float* x, size_t rows, int C, void* workspace, int* splits_out, void* stream);
int srk_bn_finalize_apply_act(const double* partials, int splits, double* stats, size_t rows, int C, float* save_mean,
                              float* save_rstd, float* running_mean, float* running_var, float momentum, float eps,
                              int64_t* num_batches_tracked, const float* x, float* y, const float* gamma, const float* beta,
                              int act, float slope, const float* prelu_weight, int prelu_n, const float* residual,
                              float* y_amax, void* stream);
int srk_bn_backward_partials_act(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                                 const float* beta, size_t rows, int C, int act, float slope, const float* prelu_weight,
                                 int prelu_n, void* workspace, int* splits_out, void* stream);
int srk_bn_backward_finalize_apply_act(const double* partials, int splits, double* dstats, double count, const float* dy,
                                       const float* x, const float* mean, const float* rstd, const float* gamma,
                                       const float* beta, float* dx, size_t rows, int C, float* dgamma, float* dbeta,
                                       int act, float slope, const float* prelu_weight, int prelu_n, float* dprelu,
                                       void* stream);

/* ---- Linear (DenseBlock: base_networks.py:7; srgan.py:66-70) -------------------------------- */
/* y[B,Out] = act(x[B,In] @ w[Out,In]^T + b) */
int srk_linear_forward(const float* x, const float* w, const float* b, float* y, int B, int In, int Out, int act,
                       float slope, void* stream);
int srk_linear_backward(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int B,
                        int In, int Out, float beta, void* stream);

/* ---- utils.img_interp (utils.py:242-269): ToPILImage -> Image.resize -> ToTensor, bit-exact ---------------------
 * x, y: dense NCHW fp32 (the reference's FloatTensor layout); values are quantised to uint8 by truncation of x*255
 * (saturating outside [0,1]), resampled with Pillow's 8-bit two-pass algorithm and returned as uint8/255.
 * SRCNN / VDSR / LapSRN call it every iteration (srcnn.py:119, vdsr.py:137, lapsrn.py:183). */
typedef enum srk_interp {
  SRK_INTERP_NEAREST = 0,
  SRK_INTERP_BILINEAR = 2,
  SRK_INTERP_BICUBIC = 3,
  SRK_INTERP_BOX = 4 /* Image.BOX: support 0.5, weight 1 on (-0.5, 0.5]; srk_img_resize_u8 only */
} srk_interp; /* PIL codes */
size_t srk_img_interp_workspace_bytes(int N, int C, int H, int W, int OH, int OW, int filter);
int srk_img_interp(const float* x_nchw, float* y_nchw, int N, int C, int H, int W, int OH, int OW, int filter,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- training-set pipeline on 8-bit images (dataset.py:51-99; torchvision's Scale / RandomCrop / flips around Pillow) ----
 * Image.resize((OW, OH), BICUBIC | BILINEAR | BOX) on 8-bit planes, bit-exact with Pillow (same two-pass resampler as
 * srk_img_interp; a pass is skipped when that axis keeps its size, as Pillow does).  x is addressed through element
 * strides (plane, row, pixel): an interleaved HWC decode buffer is read in place with (1, W*C, C).  y: planar
 * [planes][OH][OW], uint8 (out_float = 0) or float = value / 255 (out_float = 1: ToTensor). */
size_t srk_img_resize_u8_workspace_bytes(int planes, int H, int W, int OH, int OW, int filter);
int srk_img_resize_u8(const uint8_t* x, int64_t plane_stride, int64_t row_stride, int64_t px_stride, void* y,
                      int out_float, int planes, int H, int W, int OH, int OW, int filter, void* workspace,
                      size_t workspace_bytes, void* stream);
/* RandomCrop -> Image.rotate(90*rot_k, expand=True) (counter-clockwise quarter turns) -> horizontal flip -> vertical
 * flip (dataset.py:65-84) as one gather: y planar [C][crop_h or crop_w][...] uint8. */
int srk_patch_augment_u8(const uint8_t* x, int64_t plane_stride, int64_t row_stride, int64_t px_stride, uint8_t* y, int C,
                         int H, int W, int crop_x, int crop_y, int crop_w, int crop_h, int rot_k, int fliplr, int fliptb,
                         void* stream);
/* The two calls above folded into one per training patch (dataset.py:51-82): img_hwc is the decoded interleaved 8-bit
 * image [H][W][C]; scale_h / scale_w > 0 rescale the whole image first (Image.resize, BICUBIC), 0 = no rescale; then
 * crop -> rot_k quarter turns ccw -> flips into the planar patch out_planar [C][oh][ow]. */
size_t srk_patch_from_image_u8_workspace_bytes(int C, int H, int W, int scale_h, int scale_w);
int srk_patch_from_image_u8(const uint8_t* img_hwc, int C, int H, int W, int scale_h, int scale_w, int crop_x, int crop_y,
                            int crop_w, int crop_h, int rot_k, int fliplr, int fliptb, uint8_t* out_planar,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- the colour tail of test_single / test (edsr.py:276-322, utils.py:116-131), bit-exact with Pillow ----------
 * Image.convert('YCbCr') / convert('RGB') are integer table look-ups in Pillow (ConvertYCbCr.c, SCALE = 6); the closed
 * form of the tables is in csrc/color.hip.  The tables are constants of the library, built once by its compiler in IEEE
 * double; the host helpers and the kernels read the same object.
 *
 * srk_rgb_to_ycc_u8: interleaved 8-bit RGB [H][W][3] (row_stride in bytes, >= 3 W) -> any of (NULL = not wanted, at least
 *   one): y_f32 [H][W] = Y / 255.0f (ToTensor of the Y plane), y_u8 [H][W], cbcr [2][H][W] 8-bit planar (what
 *   srk_img_resize_u8 reads with plane_stride = H * W).  One pass over the image.
 * srk_ycc_to_rgb_u8: Image.merge('YCbCr', ...).convert('RGB') -> interleaved 8-bit RGB [H][W][3].  Y is EITHER y_f32 (the
 *   net's output, addressed through element strides (row, pixel); quantised like srk_float_to_u8_image on the way, the
 *   8-bit Y never goes to memory) OR y_u8 (dense [H][W]); exactly one of the two is non-NULL.  cb / cr: dense [H][W].
 * srk_float_to_u8_image: ToPILImage after clamp(0, 1) (edsr.py:305-306): (uint8)(min(max(x, 0), 1) * 255.0f), fp32
 *   product, truncation, NaN -> 0.  x: fp32 [C][H][W] through element strides (channel, row, pixel) -- a channels-last
 *   net output is read in place --, C = 1 or 3; out: interleaved [H][W][C]. */
int srk_rgb_to_ycc_u8(const uint8_t* rgb, int64_t row_stride, int H, int W, float* y_f32, uint8_t* y_u8, uint8_t* cbcr,
                      void* stream);
int srk_ycc_to_rgb_u8(const float* y_f32, int64_t y_row_stride, int64_t y_px_stride, const uint8_t* y_u8, const uint8_t* cb,
                      const uint8_t* cr, uint8_t* rgb, int H, int W, void* stream);
int srk_float_to_u8_image(const float* x, int64_t c_stride, int64_t row_stride, int64_t px_stride, uint8_t* out, int C,
                          int H, int W, void* stream);
/* The same two conversions on the HOST (pure functions, no device involved; n interleaved pixels, 3 bytes each): they
 * read the very tables the kernels get, so the arithmetic can be pinned against Pillow without a GPU. */
int srk_rgb_to_ycc_host(const uint8_t* rgb, size_t n, uint8_t* ycc);
int srk_ycc_to_rgb_host(const uint8_t* ycc, size_t n, uint8_t* rgb);

/* ---- tiled super-resolution of one picture (tiling.py; csrc/tile.hip) ------------------------------------------
 * (Added without a change of srk_version(): new entry points only, nothing existing changed.)
 * A picture is cut into equal, overlapping tiles that lie inside it, the tiles run through the net as batches, and every
 * output pixel is taken from the ONE tile that owns it.  The plan is separable; `table` is device memory, int32
 * [nty + ntx][4], the nty tile rows first, then the ntx tile columns, an entry being {input offset of the tile, first
 * owned output pixel, end of the owned output pixels, output pixel of the tile's local output pixel 0}.  Tile t =
 * row * ntx + col; a call handles tiles t0 .. t0 + n.  The kernels skip, and never dereference, a coordinate the table
 * puts outside a tile or the picture.
 *
 * srk_tile_gather: fp32 picture [C][H][W] through element strides (channel, row, pixel), C = 1 or 3 -> dense NHWC tiles
 *   out [n][th][tw][C].
 * srk_tile_stitch_f32: tile outputs [n][C][oth][otw] through element strides (tile, channel, row, pixel) -- a
 *   channels-last net output is read in place -> the owned rectangles of those tiles in the fp32 picture out [C][OH][OW].
 *   The chunks of a plan together write every pixel of out exactly once.
 * srk_tile_stitch_u8: the same walk, writing the final interleaved 8-bit picture: cb == cr == NULL: out [OH][OW][C],
 *   quantised like srk_float_to_u8_image; else C = 1 and cb / cr are dense 8-bit planes [OH][OW]: out [OH][OW][3] RGB,
 *   Y quantised and converted like srk_ycc_to_rgb_u8.  The fp32 picture is never written. */
int srk_tile_gather(const float* pic, int64_t c_stride, int64_t row_stride, int64_t px_stride, int C, int H, int W,
                    const int32_t* table, int nty, int ntx, int th, int tw, int t0, int n, float* out, void* stream);
int srk_tile_stitch_f32(const float* tiles, int64_t n_stride, int64_t c_stride, int64_t row_stride, int64_t px_stride, int C,
                        int oth, int otw, const int32_t* table, int nty, int ntx, int t0, int n, float* out, int OH, int OW,
                        void* stream);
int srk_tile_stitch_u8(const float* tiles, int64_t n_stride, int64_t c_stride, int64_t row_stride, int64_t px_stride, int C,
                       int oth, int otw, const int32_t* table, int nty, int ntx, int t0, int n, const uint8_t* cb,
                       const uint8_t* cr, uint8_t* out, int OH, int OW, void* stream);

/* ---- x8 geometric self-ensemble (sr_trainers.py self_ensemble; csrc/dihedral.hip) -------------------------------
 * (Added without a change of srk_version(): new entry points only, nothing existing changed.)
 * Variant k = 4 m + r of a picture x is T_k(x) = rot90(flip of the last axis if m, r turns); the ensemble is
 * E = (((((((y_0 + y_1) + y_2) + y_3) + y_4) + y_5) + y_6) + y_7) * 0.125 in fp32 with y_k = T_k^-1(net(T_k(x))).
 *
 * srk_dihedral_variants: fp32 pictures [N][C][H][W] through element strides (image, channel, row, pixel), C = 1 or 3 ->
 *   out, dense channels-last, 8 N images in one allocation: first 4 N images of H x W, image 4 n + j = T_k(x[n]) with
 *   k = (0, 2, 4, 6)[j]; then 4 N images of W x H, k = (1, 3, 5, 7)[j].  One launch.
 * srk_dihedral_merge_f32: the net's outputs for the two groups, even [4N][C][oh][ow] and odd [4N][C][ow][oh], each
 *   through four element strides (image, channel, row, pixel; NCHW or channels-last) -> E, dense [N][C][oh][ow].
 * srk_dihedral_merge_u8: N = 1, writing the final interleaved 8-bit picture instead: cb == cr == NULL: out [oh][ow][C],
 *   quantised like srk_float_to_u8_image; else C = 1 and cb / cr are dense 8-bit planes [oh][ow]: out [oh][ow][3] RGB,
 *   Y quantised and converted like srk_ycc_to_rgb_u8.  The fp32 mean is never written. */
int srk_dihedral_variants(const float* x, int64_t n_stride, int64_t c_stride, int64_t row_stride, int64_t px_stride, int N,
                          int C, int H, int W, float* out, void* stream);
int srk_dihedral_merge_f32(const float* even, const int64_t* even_strides, const float* odd, const int64_t* odd_strides, int N,
                           int C, int oh, int ow, float* out, void* stream);
int srk_dihedral_merge_u8(const float* even, const int64_t* even_strides, const float* odd, const int64_t* odd_strides, int C,
                          int oh, int ow, const uint8_t* cb, const uint8_t* cr, uint8_t* out, void* stream);

/* ---- steps either side of the nets ------------------------------------------------
 * utils.PSNR (utils.py:208-216): mse = mean((clamp(pred,0,1) - gt)^2) over all elements, *psnr_out = mse == 0 ? 100 :
 * 10*log10(1/mse), on the device (the reference copies both images to the host per test image).  pred / gt are
 * addressed through element strides (n,c,h,w); NULL = NHWC-dense.  mse_out may be NULL. */
size_t srk_psnr_workspace_bytes(void);
int srk_psnr(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides, int N, int C,
             int H, int W, float* psnr_out, float* mse_out, void* workspace, void* stream);
/* SSIM (Wang, Bovik, Sheikh, Simoncelli 2004, as ssim_index.m computes it) of pred against gt, on the device.
 * (Added without a change of srk_version(): new entry points only, nothing existing changed.)
 * Window 11 x 11, separable, g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) normalised to sum 1; the five moments at the VALID
 * positions only ((H' - 10) x (W' - 10) of an H' x W' plane); C1 = (0.01 L)^2, C2 = (0.03 L)^2; the result is the plain
 * mean over all positions of all planes of all images of the call.  Moments are accumulated in double.
 * shave >= 0 crops that many pixels from each side of both tensors first (H' = H - 2 shave; no copy).  domain says what
 * enters the moments, for BOTH tensors, applied while they are read and never written to memory:
 *   SRK_SSIM_FLOAT  clamp(pred, 0, 1) against gt as it is (what srk_psnr compares; NaN in pred counts as 0), L = 1
 *   SRK_SSIM_U8     the byte of srk_float_to_u8_image, (uint8)(clamp(v, 0, 1) * 255.0f), L = 255
 *   SRK_SSIM_Y8     C == 3: those bytes through Pillow's RGB -> Y table (srk_rgb_to_ycc_u8), one plane per image;
 *                   C == 1: as SRK_SSIM_U8; any other C is refused
 * *mse_out = mean squared difference of the same pixels (all H' x W' of them) divided by L^2, *psnr_out = mse == 0 ? 100 :
 * 10 log10(1 / mse); either may be NULL.  pred / gt are addressed through element strides (n,c,h,w); NULL = NHWC-dense.
 * Per-block sums go to `workspace` (srk_ssim_workspace_bytes() bytes, contents irrelevant) and are added in a fixed
 * order: two calls on the same inputs return the same bits.  A plane under 11 x 11 after the crop is SRK_ERR_BAD_ARG.
 * srk_ssim_host: the same definition in plain C++ double on HOST pointers (no device involved), sharing the window, the
 * domains and the formula with the kernel, so the definition can be pinned without a GPU. */
enum { SRK_SSIM_FLOAT = 0, SRK_SSIM_U8 = 1, SRK_SSIM_Y8 = 2 };
size_t srk_ssim_workspace_bytes(void);
int srk_ssim(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides, int N, int C,
             int H, int W, int shave, int domain, float* ssim_out, float* psnr_out, float* mse_out, void* workspace,
             void* stream);
int srk_ssim_host(const float* pred, const int64_t* pred_strides, const float* gt, const int64_t* gt_strides, int N, int C,
                  int H, int W, int shave, int domain, double* ssim_out, double* psnr_out, double* mse_out);
/* The SSIM training loss with its gradient, one pass: *loss = 1 - mean SSIM of pred against target, dpred = grad_scale *
 * d(loss)/d(pred).  (Added without a change of srk_version(): new entry points only.)  Window, constants and the "valid
 * positions only" rule are srk_ssim's; two things differ: pred is read UNCLAMPED (a clamp would zero the gradient of every
 * out-of-range pixel; on planes within [0, 1] the loss is 1 - srk_ssim(SRK_SSIM_FLOAT)), and the domain is float, L = 1.
 * Per plane x (pred), y (target) of H x W, H, W >= 11, with G the 11 x 11 window at the (H-10) x (W-10) valid positions
 * and G^T its adjoint (a pixel gathers from the up to 11 x 11 positions whose window holds it):
 *   mx = G x, my = G y, exx = G x^2, eyy = G y^2, exy = G xy;  vx = exx - mx^2, vy = eyy - my^2, cov = exy - mx my
 *   A1 = 2 mx my + C1, A2 = 2 cov + C2, B1 = mx^2 + my^2 + C1, B2 = vx + vy + C2,  S = A1 A2 / (B1 B2)
 *   loss = 1 - mean of S over all M = N C (H-10)(W-10) positions (per plane, unweighted across channels)
 *   Pm = 2 my (A2 - A1)/(B1 B2) - 2 mx S/B1 + 2 mx S/B2,  Pxx = -S / B2,  Pxy = 2 A1 / (B1 B2)
 *   d loss / d x = -(1/M) (G^T Pm + 2 x G^T Pxx + y G^T Pxy)
 * All of it in double up to the fp32 stores.  Conventions of srk_loss_forward_backward: pred / dpred NHWC-dense, target
 * through element strides (n,c,h,w) (NULL = NHWC-dense), dpred may be NULL (loss only), `workspace` of
 * srk_ssim_loss_workspace_bytes() bytes (contents irrelevant).  No atomics: two calls return the same bits.  A NaN in pred
 * propagates.  A plane under 11 x 11 is SRK_ERR_BAD_ARG.
 * srk_ssim_loss_host: the same definition in plain C++ double on HOST pointers, sharing window and formula with the
 * kernel; *loss and dpred (NHWC-dense, may be NULL) are doubles. */
size_t srk_ssim_loss_workspace_bytes(void);
int srk_ssim_loss_forward_backward(const float* pred, const float* target, const int64_t* target_strides, int N, int C,
                                   int H, int W, float grad_scale, float* loss, float* dpred, void* workspace,
                                   void* stream);
int srk_ssim_loss_host(const float* pred, const float* target, const int64_t* target_strides, int N, int C, int H, int W,
                       double grad_scale, double* loss, double* dpred);
/* The frequency-domain training loss with its gradient: an L1 on the full 2-D Fourier spectrum of d = pred - target, per
 * plane (BasicSR's FFTLoss: L1Loss(view_as_real(fft2(pred)), view_as_real(fft2(target)))).  (Added without a change of
 * srk_version(): new entry points only.)  pred, target [N,C,H,W] fp32, 1 <= H, W <= SRK_FFT_LOSS_MAX_DIM, M = N*C*H*W,
 * d formed in double from the fp32 values:
 *   F[n,c,u,v] = s * sum_{y,x} d[n,c,y,x] * exp(-2 pi i (u y / H + v x / W))     s = `scale`: 1 ("backward") or
 *   loss       = (1 / (2 M)) * sum_{n,c,u,v} (|Re F| + |Im F|)                       1 / sqrt(H W) ("ortho")
 *   G          = sign(Re F) + i sign(Im F),  sign(0) = 0
 *   dpred[n,c,y,x] = grad_scale * (s / (2 M)) * Re sum_{u,v} G[n,c,u,v] * exp(+2 pi i (u y / H + v x / W))
 * No gradient goes to target; a NaN in pred propagates (to the loss and to its own plane's gradient).  The DFT is dense
 * and fp64 up to the fp32 stores of dpred and *loss.  Its twiddles are DATA from one host function:
 * srk_dft_table_host(n, cos_sin) fills cos_sin[2k] = cos(2 pi k / n), cos_sin[2k+1] = sin(2 pi k / n), k = 0 .. n-1;
 * wherever 4k is a multiple of n the entries are exactly 0 and +-1, and entry n - k is the conjugate of entry k to the
 * bit.  Kernels, host twin and tests all address these values by (u * y) mod n, so for a real d Im F is an exact zero
 * at the self-conjugate bins (2u = 0 mod H and 2v = 0 mod W) and the sign there is 0.
 * `tables` (device): the table of H followed by the table of W, 2 * (H + W) doubles.  Conventions of
 * srk_ssim_loss_forward_backward: pred / dpred NHWC-dense, target through element strides (n,c,h,w) (NULL = NHWC-dense),
 * dpred may be NULL (loss only), `workspace` of srk_fft_loss_workspace_bytes(N, C, H, W) bytes (contents irrelevant; 0
 * for dims the call refuses).  No atomics: two calls return the same bits.  H or W beyond SRK_FFT_LOSS_MAX_DIM is
 * SRK_ERR_UNSUPPORTED; null pointers, non-positive dims and a scale that is not positive and finite are SRK_ERR_BAD_ARG,
 * all before anything is launched.
 * srk_fft_loss_host: the same definition in plain C++ double on HOST pointers (full spectrum, no mirror), sharing table
 * and arithmetic (csrc/fft_loss_common.h) with the kernels; *loss and dpred (NHWC-dense, may be NULL) are doubles. */
#define SRK_FFT_LOSS_MAX_DIM 256
int srk_dft_table_host(int n, double* cos_sin);
size_t srk_fft_loss_workspace_bytes(int N, int C, int H, int W);
int srk_fft_loss_forward_backward(const float* pred, const float* target, const int64_t* target_strides, int N, int C,
                                  int H, int W, const double* tables, double scale, float grad_scale, float* loss,
                                  float* dpred, void* workspace, void* stream);
int srk_fft_loss_host(const float* pred, const float* target, const int64_t* target_strides, int N, int C, int H, int W,
                      double scale, double grad_scale, double* loss, double* dpred);
/* utils.norm / utils.denorm (utils.py:219-239; torchvision Normalize = sub_(mean).div_(std)):
 * y[e] = (x[e] - sub[c]) / div[c], c = (e / inner) % C (inner = H*W for NCHW storage, 1 for NHWC), optionally clamped
 * to [0,1] (denorm's non-VGG branch).  sub_host / div_host are HOST arrays of C <= 8 floats. Bit-equal to torch. */
int srk_channel_affine(const float* x, float* y, size_t n, int C, size_t inner, const float* sub_host,
                       const float* div_host, int clamp01, void* stream);
/* torch.nn.Upsample(scale_factor=r, mode='nearest') of Upsample2xBlock('rnc') (base_networks.py:204-210), NHWC:
 * y[n,oy,ox,c] = x[n,oy/r,ox/r,c]; backward: dx = sum of each r x r block of dy. */
int srk_upsample_nearest_forward(const float* x, float* y, int N, int H, int W, int C, int r, void* stream);
int srk_upsample_nearest_backward(const float* dy, float* dx, int N, int H, int W, int C, int r, void* stream);
/* nn.MaxPool2d(2, 2) of the VGG19 feature extractor (srgan.py:84-90: vgg19.features[:9] holds one), NHWC, floor mode:
 * y [N, H/2, W/2, C].  The reference evaluates the VGG loss on detached tensors (srgan.py:302-305): forward only there. */
int srk_maxpool2x2_forward(const float* x, float* y, int N, int H, int W, int C, void* stream);
/* Its gradient, for a perceptual loss that trains (ops.perceptual_loss): x [N,H,W,C] the pool's input, dy [N,H/2,W/2,C],
 * dx [N,H,W,C].  The winner of each window is recomputed from x -- ATen's: the first maximum in (row, column) scan order
 * -- and receives dy; every other element, the trailing row / column of an odd H / W included, is written as zero:
 * every dx element exactly once, no atomics, nothing to clear before the call.  16-byte accesses when C % 4 == 0 and the
 * three pointers are 16-byte aligned, else one float at a time.  relu_input != 0: x is the output of a fused conv + ReLU;
 * windows whose maximum is <= 0 route nothing, so dx is already what that conv's (x > 0) mask would leave.
 * NaN in x is out of scope (the forward propagates it; the gradient's winner is then unspecified). */
int srk_maxpool2x2_backward(const float* x, const float* dy, float* dx, int N, int H, int W, int C, int relu_input,
                            void* stream);

/* ---- training degradations on the loader's 8-bit patches (data.Degradation; csrc/degrade.hip) -------------------
 * (Added without a change of srk_version(): new entry points only, nothing existing changed.)
 * The classical degradation model LR = (HR * k) shrunk + n, defined to the bit so that a numpy restatement gives the
 * same bytes.
 *
 * srk_blur_u8: x, y dense 8-bit [B][planes_per_patch][H][W]; w fp64 [B][K][K], one table per patch, row-major (i, j).
 *   y = floor(clamp(sum_{i,j} w[b][i][j] * x[b][c][yy + i - r][xx + j - r], 0, 255) + 0.5), r = K / 2, borders mirrored
 *   without repeating the edge pixel (reflect-101).  The sum is fp64, taps added in row-major (i, j) order; a table
 *   narrower than K sits centred among zeros (0.0 * p leaves the sum unchanged), and the delta table returns x bit for bit.
 *   SRK_ERR_INVALID before anything is launched: null pointer, K even or outside [3, 21], H or W <= K / 2.
 * srk_noise_u8: x 8-bit, y float, both dense [B][elems_per_patch]; sigma fp64 [B] on the device, in 8-bit levels.
 *   y[e] = float(clamp(floor(x[e] + sigma[b] * z[e] + 0.5), 0, 255)) / 255.0f (the division srk_img_resize_u8 makes with
 *   out_float = 1; sigma = 0 gives x / 255 exactly).  z[e] is lane e & 3 of the four normals of group q = e >> 2, e the
 *   linear index over the whole call: Philox4x32-10 under key (seed & 0xffffffff, seed >> 32) on counter
 *   (q & 0xffffffff, q >> 32, 0, 0) gives words x0..x3; with u(x) = (x + 0.5) * 2^-32 and rad(x) = sqrt(-2 ln u(x)):
 *   n0 = rad(x0) cos(2 pi u(x1)), n1 = rad(x0) sin(2 pi u(x1)), n2 = rad(x2) cos(2 pi u(x3)), n3 = rad(x2) sin(2 pi u(x3)),
 *   all in fp64.
 * Host-only twins, pure functions that need no device:
 * srk_blur_weights_host: w[i][j] = exp(-0.5 * (u^2 / s1^2 + v^2 / s2^2)), u = cos(theta) x + sin(theta) y,
 *   v = -sin(theta) x + cos(theta) y, x = j - K / 2, y = i - K / 2, divided by the table's sum (row-major, fp64).
 *   K odd in [1, 21], s1, s2 > 0.
 * srk_noise_normals_host: z[k] = the normal of element first_elem + k under `seed`, from the very Philox and Box-Muller
 *   body the kernel compiles (csrc/degrade_common.h); the two sides differ by what their libm's do, an ulp.
 * srk_philox4x32_10_host: that body's generator alone, out[0..3] = Philox4x32-10 of counter[0..3] under key[0..1], so
 *   the published known-answer vectors (any counter, any key) can be checked against the code the kernel runs. */
int srk_blur_u8(const uint8_t* x, uint8_t* y, const double* w, int planes_per_patch, int B, int H, int W, int K,
                void* stream);
int srk_noise_u8(const uint8_t* x, float* y, const double* sigma, uint64_t seed, int B, int64_t elems_per_patch,
                 void* stream);
int srk_blur_weights_host(double s1, double s2, double theta, int K, double* w);
int srk_noise_normals_host(uint64_t seed, int64_t first_elem, int64_t n, double* z);
int srk_philox4x32_10_host(const uint32_t* counter, const uint32_t* key, uint32_t* out);

/* ---- JPEG artefacts on the loader's 8-bit patches (data.Degradation's last stage; csrc/jpeg.hip) -------------------
 * (Additive again: new entry points only, srk_version() and everything existing unchanged.)
 * y = decode(encode(x, Q)): libjpeg's baseline round trip at quality Q without its lossless entropy coder, a pure function
 * from bytes to bytes in int32 arithmetic (>> arithmetic, DESCALE(v, n) = (v + (1 << (n - 1))) >> n); DESIGN.md 24 and
 * csrc/jpeg_common.h spell out every step.  In short, per picture of C dense 8-bit planes [H][W]:
 *   tables    Annex K (luminance, chrominance), t = clamp((base * s + 50) / 100, 1, 255), s = 5000 / Q below 50, else
 *             200 - 2 Q, Q clamped to 1..100;
 *   colour    color = 1 (C = 3, planes R, G, B): libjpeg's 16-bit fixed-point RGB -> YCbCr; color = 0: the planes are
 *             Y, Cb, Cr as they stand; C = 1: a grey picture, luminance table only;
 *   shrink    subsampling = 1 (4:2:0): 2 x 2 means with bias 1 / 2 on even / odd columns; source columns replicated to a
 *             multiple of 16, an odd height's last row once more, then the SHRUNK plane's last row replicated to a
 *             multiple of 8.  subsampling = 0 (4:4:4), and luma always: last row / column replicated to a multiple of 8;
 *   DCT       jfdctint on sample - 128 (rows, then columns), q = sign(c) * ((|c| + (d >> 1)) / d) with d = t << 3, the
 *             coefficient q * t, jidctint (columns, then rows), + 128, clamped to 0..255 (libjpeg's range-limit table
 *             wraps far outside its range; the one deliberate departure);
 *   expand    4:2:0: libjpeg's "fancy" triangle filter over the ceil(H/2) x ceil(W/2) real chroma samples, neighbours
 *             clamped to them; chroma planes of at most two columns (W <= 4) are replicated instead, as libjpeg does;
 *   colour    color = 1: libjpeg's fixed-point YCbCr -> RGB, clamped.
 *   Q = 0 means "not compressed": the patch comes out bit for bit.
 * srk_jpeg_u8: x dense 8-bit [B][C][H][W]; quality fp64 [B] on the device, whole numbers (they ride in the loader's one
 *   fp64 parameter copy), one per patch; y 8-bit of x's shape, or with out_float fp32 byte / 255.0f -- the division
 *   srk_img_resize_u8 and srk_noise_u8 make.  SRK_ERR_INVALID before anything is launched: null pointer, C not 1 or 3,
 *   color = 1 with C = 1, subsampling outside {0, 1}, a size <= 0.  With C = 1 subsampling has nothing to act on.
 * srk_noise_u8_bytes: srk_noise_u8 with the clamped 8-bit level itself as the result (the same kernel body), so that
 *   bytes / 255.0f are srk_noise_u8's bits and the JPEG stage can follow the noise.
 * Host-only twins, pure functions that need no device:
 * srk_jpeg_quant_table_host: out[0..63] = the table (chroma 0 / 1) of `quality` in natural order.
 * srk_jpeg_u8_host: the whole round trip as a loop over the very bodies the kernel compiles; quality int [B] on the host. */
int srk_jpeg_u8(const uint8_t* x, void* y, const double* quality, int C, int B, int H, int W, int subsampling, int color,
                int out_float, void* stream);
int srk_noise_u8_bytes(const uint8_t* x, uint8_t* y, const double* sigma, uint64_t seed, int B, int64_t elems_per_patch,
                       void* stream);
int srk_jpeg_quant_table_host(int quality, int chroma, int* out);
int srk_jpeg_u8_host(const uint8_t* x, uint8_t* y, const int* quality, int C, int B, int H, int W, int subsampling,
                     int color);

/* ---- Real-ESRGAN's second-order degradation and USM targets (data.Degradation2) ----------------------
 * (Additive: new entry points and SRK_INTERP_BOX only, srk_version() and everything existing unchanged.)
 * Every stage is 8 bits in, 8 bits out and defined to the byte; tests/degrade2_ref.py restates each in numpy.
 *
 * srk_blur_table_host: the normalised K x K fp64 table (row-major (i, j), x = j - K / 2, y = i - K / 2) of one kind, K odd
 *   in [7, 21], for srk_blur_u8 to take unchanged.  With u = cos(theta) x + sin(theta) y, v = -sin(theta) x + cos(theta) y
 *   and q = u^2 / s1^2 + v^2 / s2^2:  GAUSS exp(-0.5 q);  GGAUSS exp(-0.5 q^beta);  PLATEAU 1 / (1 + q^beta);  SINC the
 *   circular low-pass cutoff * J1(cutoff r) / (2 pi r), r = sqrt(x^2 + y^2), cutoff^2 / (4 pi) at r = 0 (J1 is libm's j1;
 *   the table has negative entries, which srk_blur_u8's clamp covers).  Each table is divided by its compensated sum;
 *   the centre tap then takes up what the rounded entries' sum still lacks from 1, so a table sums to 1 within an ulp.
 *   Arguments a kind does not use are ignored.  SRK_ERR_INVALID: null pointer, K even or outside [7, 21], a sigma, beta or
 *   cutoff that its kind needs and that is not positive.
 * srk_poisson_cdf_host: cdf[256][KT] fp64, cdf[L][k] = P(Pois(L * peak / 255) <= k) from the running product
 *   pmf(k) = pmf(k - 1) * lambda / k (pmf(0) = exp(-lambda)) under a compensated sum, clamped to 1, made non-decreasing,
 *   the last column forced to 1.0.  The chain uses peak 256, KT = SRK_POISSON_KT = 448.
 * srk_noise2_u8: x, y dense 8-bit [B][C][H][W], C 1 or 3; mode, gray, amount fp64 [B] and cdf fp64 [256][448] on the
 *   device.  Words and normals are srk_noise_u8's (Philox4x32-10, Box-Muller in fp64) with `stage` (0, 1 or 2) in counter
 *   word 2; stage 0 is srk_noise_u8's own stream.  An element's generator index is its linear index e over the call
 *   (colour noise) or its pixel's index b * H * W + y * W + x (gray[b] != 0: one draw per pixel, shared by the planes); it
 *   takes lane (index & 3) of group (index >> 2).  Per patch:
 *     mode 0 (SRK_NOISE2_OFF)      y = x;
 *     mode 1 (SRK_NOISE2_GAUSS)    y = clamp(floor(x + amount * z + 0.5), 0, 255), z the index's normal;
 *     mode 2 (SRK_NOISE2_POISSON)  k = the smallest column with u(word) <= cdf[L][k] (binary search), L the byte itself,
 *                                  or with gray noise the pixel's gray level: floor((R + G + B) / 3 + 0.5) with
 *                                  color != 0, plane 0 (the Y of Y, Cb, Cr planes) with color = 0, the byte with C = 1; y = clamp(floor(x + amount * (k * 255 / 256 - L) + 0.5), 0, 255).
 *   All arithmetic is fp64, products and sums uncontracted; the device evaluates no transcendental for Poisson.
 *   SRK_ERR_INVALID before anything is launched: null pointer, C not 1 or 3, a size <= 0, stage outside 0..2.
 * srk_noise2_u8_host: the same body (csrc/degrade_common.h) looped on the host, all pointers host memory.
 * srk_usm_table_host: g[i] = exp(-(i - K / 2)^2 / (2 sigma^2)) normalised as srk_blur_table_host's, K odd in [1, 51];
 *   sigma <= 0 means cv2's 0.3 * ((K - 1) * 0.5 - 1) + 0.8 (8.0 at K = 51).
 * srk_usm_u8: Real-ESRGAN's USMSharp on dense 8-bit planes x [B][C][H][W] -> y; g fp64 [K] on the device.  With blur(A)
 *   the separable pass of g over rows then columns (fp64 intermediate unrounded, taps added in index order from 0, borders
 *   reflect-101):  Bl = blur(x);  R = x - Bl;  M = |R| > threshold;  S = blur(M);  sharp = clamp(x + weight * R, 0, 255);
 *   y = floor(clamp(S * sharp + (1 - S) * x, 0, 255) + 0.5).  fp64 throughout, uncontracted; no atomics; the workspace
 *   (srk_usm_u8_workspace_bytes) holds R and M between the two launches.  SRK_ERR_INVALID before anything is launched:
 *   null pointer, K even or outside [1, 51], C not 1 or 3, H or W <= K / 2; SRK_ERR_WORKSPACE: workspace too small.
 * srk_usm_u8_host: the same bodies (csrc/usm_common.h) looped on the host. */
enum { SRK_BLUR_GAUSS = 0, SRK_BLUR_GGAUSS = 1, SRK_BLUR_PLATEAU = 2, SRK_BLUR_SINC = 3 };
enum { SRK_NOISE2_OFF = 0, SRK_NOISE2_GAUSS = 1, SRK_NOISE2_POISSON = 2 };
enum { SRK_POISSON_KT = 448, SRK_USM_MAX_K = 51 };
int srk_blur_table_host(int kind, int K, double s1, double s2, double theta, double beta, double cutoff, double* w);
int srk_poisson_cdf_host(double peak, int KT, double* cdf);
int srk_noise2_u8(const uint8_t* x, uint8_t* y, const double* mode, const double* gray, const double* amount,
                  const double* cdf, uint64_t seed, int stage, int B, int C, int H, int W, int color, void* stream);
int srk_noise2_u8_host(const uint8_t* x, uint8_t* y, const double* mode, const double* gray, const double* amount,
                       const double* cdf, uint64_t seed, int stage, int B, int C, int H, int W, int color);
int srk_usm_table_host(int K, double sigma, double* g);
size_t srk_usm_u8_workspace_bytes(int B, int C, int H, int W);
int srk_usm_u8(const uint8_t* x, uint8_t* y, const double* g, int K, double weight, double threshold, int B, int C, int H,
               int W, void* workspace, size_t workspace_bytes, void* stream);
int srk_usm_u8_host(const uint8_t* x, uint8_t* y, const double* g, int K, double weight, double threshold, int B, int C,
                    int H, int W);

/* ---- Channel attention: the gate of RCAN's residual channel attention block (csrc/ca.hip, csrc/ca_common.h) ---------
 * (Additive again: new entry points only, srk_version() and everything existing unchanged.)
 * t, x, y, g, dt dense NHWC [N][H][W][C]; W1 [Cr][C], b1 [Cr], W2 [C][Cr], b2 [C] (1x1 conv filters, [out][in]).
 *   m[n][c] = (1 / HW) sum_hw t[n][h][w][c]       h[n] = relu(W1 m[n] + b1)       s[n] = sigmoid(W2 h[n] + b2)
 *   y = t * s[n][c] (+ x)                          x == NULL: no skip
 * and from g = dL/dy (dL/dx is g itself: the caller hands it on, no kernel and no argument here)
 *   ds[n][c] = sum_hw g * t      da = ds * s * (1 - s)      dh = (W2^T da) where h > 0      dm = W1^T dh
 *   dt = g * s[n][c] + dm[n][c] / HW
 *   dW2 = sum_n da_n h_n^T   db2 = sum_n da_n   dW1 = sum_n dh_n m_n^T   db1 = sum_n dh_n
 * Both sums over HW are fp64 sums of exact products through srk_channel_attention_splits() per-block partials a sample,
 * added up in index order; the MLP and its backward are fp64; the sums over n run in index order.  No atomics: two calls
 * on the same inputs give the same bits.  Only y = fma(t, s, x) and dt = fma(g, s, dm / HW) are fp32.
 * Supported: C <= SRK_CA_MAX_C, Cr <= SRK_CA_MAX_CR (SRK_ERR_UNSUPPORTED beyond, the message names the limit); 16-byte
 * accesses where C % 4 == 0 and the tensors are 16-byte aligned, else a 4-byte path.  SRK_ERR_BAD_ARG: a null pointer, a
 * size <= 0, Cr > C.  SRK_ERR_WORKSPACE: fewer than srk_channel_attention_workspace() bytes.
 * srk_channel_attention_splits: the partial blocks per sample the planner chooses (a negative status for bad sizes).
 * srk_channel_attention_workspace: bytes either direction needs (0 for bad sizes); 8-byte aligned, contents undefined.
 * srk_channel_attention_forward: two launches.  m [N][C], h [N][Cr], s [N][C] are what the backward reads; all three
 *   NULL when no backward follows.
 * srk_channel_attention_backward: three launches (two when dw1, db1, dw2 and db2 are all NULL; each may be NULL alone).
 *   out = beta * out + gradient for the four parameter gradients; beta == 0 never reads out.
 * srk_channel_attention_host: forward (and, with g != NULL, backward) on host pointers with everything after the fp32
 *   inputs in double, from the very MLP bodies the kernels compile. */
#define SRK_CA_MAX_C 256
#define SRK_CA_MAX_CR 64
int srk_channel_attention_splits(int N, int H, int W, int C);
size_t srk_channel_attention_workspace(int N, int H, int W, int C);
int srk_channel_attention_forward(const float* t, const float* x, const float* w1, const float* b1, const float* w2,
                                  const float* b2, int N, int H, int W, int C, int Cr, float* y, float* m, float* h, float* s,
                                  void* workspace, size_t workspace_bytes, void* stream);
int srk_channel_attention_backward(const float* g, const float* t, const float* w1, const float* w2, const float* m,
                                   const float* h, const float* s, int N, int H, int W, int C, int Cr, float* dt, float* dw1,
                                   float* db1, float* dw2, float* db2, float beta, void* workspace, size_t workspace_bytes,
                                   void* stream);
int srk_channel_attention_host(const float* t, const float* x, const float* w1, const float* b1, const float* w2,
                               const float* b2, const float* g, int N, int H, int W, int C, int Cr, double* y, double* dt,
                               double* dw1, double* db1, double* dw2, double* db2);

/* ---- LPIPS (Zhang et al. 2018, the VGG variant): the distance of one tapped layer (csrc/lpips.hip, lpips_common.h) ----
 * (Additive again: new entry points only, srk_version() and everything existing unchanged.)
 * f0 (the prediction's features), f1 (the target's) and df0 dense NHWC [N][H][W][C]; w [C] the layer's 1 x 1 weights.
 * Per pixel, the norms over its channels:
 *   a = ||f0||_2 + 1e-10      b = ||f1||_2 + 1e-10      q[c] = f0[c] / a - f1[c] / b      d = sum_c w[c] q[c]^2
 * value[n] = the mean of d over the sample's HW pixels; LPIPS[n] = the sum of the L layers' values; the scalar their mean
 * over n.  The normalised values are subtracted (not the expanded quadratic form): f0 == f1 gives exactly 0 and a zero
 * gradient.  The gradient goes to f0 only, with r = ||f0||_2:
 *   dd/df0[k] = 2 w[k] q[k] / a - f0[k] / (a^2 r) * sum_c 2 w[c] q[c] f0[c]      the second term is 0 where r == 0
 * (its limit, and the subgradient of a vector norm at the origin; a ReLU map has such pixels).
 * Every feature element is read once (the lanes that share a pixel hold its channels in registers) unless a lane would
 * hold more than 8 channel groups (C > 2048, or C > 512 on the 4-byte path), when the pixel is read twice.  The per-pixel
 * sums and the sum over pixels are fp64 in a fixed order, through per-block partials; no atomics: two calls on the same
 * inputs give the same bits.  Any C, H, W >= 1; 16-byte accesses where C % 4 == 0 and f0, f1, w (and df0) are 16-byte
 * aligned, else a 4-byte path.  SRK_ERR_BAD_ARG before anything is read: a null pointer, a size <= 0, a row outside the
 * table.  SRK_ERR_WORKSPACE: fewer than srk_lpips_layer_workspace() bytes.
 * srk_lpips_layer_workspace: bytes the forward needs (0 for bad sizes); 8-byte aligned, contents undefined.
 * srk_lpips_layer_blocks: the partial blocks per sample of the 16-byte (vec = 1) or the 4-byte path (a negative status for
 *   bad sizes).
 * srk_lpips_layer_forward: two launches; writes row `row` of the fp64 table [L][N]: table[row][n] = value[n].
 * srk_lpips_finish: one launch; the L rows added in order: values[n] (fp32) and mean, their mean over n (either may be
 *   NULL), and gvec[n] = seed / N (may be NULL), the per-sample upstream gradients of the scalar with the loss weight
 *   `seed` folded in -- what the layer backwards take.
 * srk_lpips_layer_backward: one launch, no workspace; recomputes the norms from f0 and f1 and writes every element of
 *   df0 = gout[n] / HW * dd/df0 once.  gout fp64 [N] on the device.
 * srk_lpips_layer_host: the same on host pointers in double throughout, from the very per-pixel bodies the kernels
 *   compile; value [N]; gout and df0 both NULL: forward only. */
size_t srk_lpips_layer_workspace(int N, int H, int W, int C);
int srk_lpips_layer_blocks(int N, int H, int W, int C, int vec);
int srk_lpips_layer_forward(const float* f0, const float* f1, const float* w, int N, int H, int W, int C, int row, int L,
                            double* table, void* workspace, size_t workspace_bytes, void* stream);
int srk_lpips_finish(const double* table, int L, int N, double seed, float* values, float* mean, double* gvec, void* stream);
int srk_lpips_layer_backward(const float* f0, const float* f1, const float* w, const double* gout, int N, int H, int W, int C,
                             float* df0, void* stream);
int srk_lpips_layer_host(const float* f0, const float* f1, const float* w, const double* gout, int N, int H, int W, int C,
                         double* value, double* df0);

/* ---- Convolution over channel slices: dense connectivity without a concatenation (csrc/dense.hip, dense_common.h) ----
 * (Additive again: new entry points and one new struct, srk_version() and everything existing unchanged.)
 * A stride-1 "same" convolution, K in {1, 3}, pad (K - 1) / 2, NHWC fp32, whose input channels are the concatenation
 * [A | B] of up to two SLICES and whose Cout results go to a slice.  A slice is a pointer to its first channel of pixel 0
 * plus the pixel stride `ld` of the buffer it lives in, in floats (ld >= its channels): pixel p = (n * H + h) * W + w of the
 * slice starts at ptr + p * ld.  CB == 0: one source (B and ldB are ignored).  W is [Cout][CA + CB][K][K] in torch's order,
 * its input channels in the order of torch.cat((A, B), 1); it is read as it is, there is no packed form.
 *   forward          y = act(conv([A | B]; W) + bias) (+ residual)       act: SRK_ACT_NONE / _RELU / _LRELU (slope)
 *   backward_data    g = dy * act'(y_saved);  dA = betaA * dA + (conv^T(g))[:CA] (+ add);  dB = betaB * dB + (conv^T(g))[CA:]
 *   backward_weight  dW = beta * dW + sum_p [A | B]^T g;  db = beta * db + sum_p g
 * y / y_saved share ldY, dy has ldDy, residual ldR, dA / dB ldDA / ldDB, add ldAdd.  y_saved is read only where act is not
 * SRK_ACT_NONE (it may be NULL otherwise).  dA or dB may be NULL: that part is not computed.  Each beta is 0 (the
 * destination may hold anything, NaN included: it is not read) or 1.  Slices of one buffer may be read and written by
 * the same call as long as their channels are disjoint (dy and dB are both slices of the growth-gradient buffer).
 * Only the slices' own channels are ever read or written.
 * Arithmetic: v_mfma_f32_16x16x32_bf16 on the exact operand splits of bf16_frag.h, fp32 accumulation; terms = 3 (x = h + m,
 * products hh + hm + mh: the SRK_ALGO_MFMA_BF16X3 class, ~5e-6) or 6 (x = h + m + l, six products: the fp32-faithful
 * SRK_ALGO_MFMA_BF16X6 class).  The weight gradient's sum over N * H * W is split into srk_dense_plan.splits pixel ranges
 * whose partials a second launch adds in index order: no atomics, two calls give the same bits.
 * Supported: CA, CB, Cout multiples of SRK_DENSE_CHANNEL_MULTIPLE, Cout <= SRK_DENSE_MAX_COUT, every ld a multiple of 4 and
 * every pointer 16-byte aligned; anything else is SRK_ERR_UNSUPPORTED and the message names the number.  SRK_ERR_BAD_ARG:
 * a null pointer, a size <= 0, terms not 3 or 6, another activation, a beta that is not 0 or 1.
 * srk_dense_conv_supported: 1 / 0 for the descriptor alone (strides and sizes; pointers are checked by the calls).
 * srk_dense_conv_plan: what the planner decided (a negative status for a refused descriptor).
 * srk_dense_conv_workspace_bytes: bytes backward_weight needs (0 for a refused descriptor); contents undefined.
 * srk_dense_conv_forward / _backward_data: one launch.  srk_dense_conv_backward_weight: two.
 * srk_dense_conv_host: the same three directions (direction 0 / 1 / 2) as plain loops on host pointers with fp64
 *   accumulation, through the same addressing and the same betas; the arguments a direction does not use may be NULL. */
#define SRK_DENSE_CHANNEL_MULTIPLE 16
#define SRK_DENSE_MAX_COUT 64
typedef struct srk_dense_desc {
  int32_t N, H, W;
  int32_t K;                 /* 1 or 3 */
  int32_t CA, CB, Cout;
  int32_t ldA, ldB, ldY;     /* pixel strides, in floats: sources, and the destination slice (= the saved output's) */
  int32_t ldR;               /* residual (forward) */
  int32_t ldDy, ldDA, ldDB;  /* output gradient, and the two source gradients */
  int32_t ldAdd;             /* the slice added into dA */
  int32_t act;               /* SRK_ACT_NONE / SRK_ACT_RELU / SRK_ACT_LRELU */
  float slope;               /* SRK_ACT_LRELU */
  int32_t terms;             /* 3 or 6 */
} srk_dense_desc;
typedef struct srk_dense_plan {
  uint32_t struct_size;      /* sizeof(srk_dense_plan) of the caller */
  int32_t pix_tiles;         /* 16-pixel tiles a wave of the forward / data-gradient kernel owns */
  int32_t splits;            /* pixel ranges of the weight gradient */
  int64_t split_pixels;      /* pixels per range */
  uint64_t ws_bytes;         /* = srk_dense_conv_workspace_bytes */
  uint64_t partial_floats;   /* floats one range's partials take: Cout * (CA + CB) * K * K + Cout */
} srk_dense_plan;
int srk_dense_conv_supported(const srk_dense_desc* d);
int srk_dense_conv_plan(const srk_dense_desc* d, srk_dense_plan* plan);
size_t srk_dense_conv_workspace_bytes(const srk_dense_desc* d);
int srk_dense_conv_forward(const srk_dense_desc* d, const float* A, const float* B, const float* W, const float* bias,
                           const float* residual, float* y, void* stream);
int srk_dense_conv_backward_data(const srk_dense_desc* d, const float* dy, const float* y_saved, const float* W, float* dA,
                                 float betaA, float* dB, float betaB, const float* add, void* stream);
int srk_dense_conv_backward_weight(const srk_dense_desc* d, const float* A, const float* B, const float* dy,
                                   const float* y_saved, float* dW, float* db, float beta, void* workspace,
                                   size_t workspace_bytes, void* stream);
int srk_dense_conv_host(const srk_dense_desc* d, int direction, const float* A, const float* B, const float* W,
                        const float* bias, const float* residual, float* y, const float* dy, const float* add, float* dA,
                        float betaA, float* dB, float betaB, float* dW, float* db, float beta);

/* ---- Slice convolution with a scaled output and two scaled skips: the RRDB epilogues (csrc/dense.hip) ----
 * (Additive again: new entry points and one new struct, srk_version(), srk_dense_desc and every srk_dense_* above unchanged.)
 * The convolution of srk_dense_desc with a caller-sized srk_dense_epilogue `e` (NULL: s = r1 = a1 = 1, no R2):
 *   forward          y = s * act(conv([A | B]; W) + bias) + r1 * R1 + r2 * R2
 *   backward_data    g = s * dy * act'(y_saved);  dA = betaA * dA + (conv^T(g))[:CA] + a1 * add;  dB as srk_dense_conv_backward_data
 *   backward_weight  the same g: dW = beta * dW + sum_p [A | B]^T g;  db = beta * db + sum_p g
 * R1 (pixel stride desc.ldR) and R2 (pixel stride e->ldR2) are optional slices of Cout channels; either may be NULL.
 * With an activation, y_saved must carry the sign of the activation's own output: s > 0 and no skip (the RRDB's scaled
 * convolutions have no activation).  s = r1 = 1 with R2 = NULL gives the bits of srk_dense_conv_forward; s = a1 = 1 those of
 * srk_dense_conv_backward_data / _backward_weight.  One launch each (backward_weight: two), the launch geometry, the
 * workspace and the planner of the plain entry points; 16-byte accesses in every epilogue; no atomics.
 * SRK_ERR_BAD_ARG: e->struct_size smaller than the struct, a scale that is not finite.
 * srk_dense_conv_host_ex: srk_dense_conv_host plus R2 and the epilogue, fp64 accumulation, the same addressing. */
typedef struct srk_dense_epilogue {
  uint32_t struct_size;      /* sizeof(srk_dense_epilogue) of the caller */
  float s;                   /* forward: scale of act(conv + bias); both gradients: scale of dy */
  float r1, r2;              /* forward: scales of R1 and R2 */
  int32_t ldR2;              /* forward: pixel stride of R2, in floats */
  float a1;                  /* backward_data: scale of `add` */
} srk_dense_epilogue;
int srk_dense_conv_forward_ex(const srk_dense_desc* d, const float* A, const float* B, const float* W, const float* bias,
                              const float* R1, const float* R2, const srk_dense_epilogue* e, float* y, void* stream);
int srk_dense_conv_backward_data_ex(const srk_dense_desc* d, const float* dy, const float* y_saved, const float* W, float* dA,
                                    float betaA, float* dB, float betaB, const float* add, const srk_dense_epilogue* e,
                                    void* stream);
int srk_dense_conv_backward_weight_ex(const srk_dense_desc* d, const float* A, const float* B, const float* dy,
                                      const float* y_saved, float* dW, float* db, float beta, const srk_dense_epilogue* e,
                                      void* workspace, size_t workspace_bytes, void* stream);
int srk_dense_conv_host_ex(const srk_dense_desc* d, int direction, const float* A, const float* B, const float* W,
                           const float* bias, const float* R1, const float* R2, const srk_dense_epilogue* e, float* y,
                           const float* dy, const float* add, float* dA, float betaA, float* dB, float betaB, float* dW,
                           float* db, float beta);

/* ---- Relativistic average GAN loss: ESRGAN's adversarial term (csrc/ragan.hip, csrc/ragan_common.h) -------------------
 * (Additive again: new entry points only, srk_version() and everything existing unchanged.)
 * real, fake: B discriminator LOGITS each ([B] or [B, 1], dense).  mr = mean(real), mf = mean(fake), a_i = real_i - mf,
 * b_i = fake_i - mr, sp(x) = max(x, 0) + log1p(exp(-|x|)):
 *   discriminator (for_generator == 0)   L = 1/(2B) sum_i [sp(-a_i) + sp(b_i)]
 *   generator     (for_generator != 0)   L = 1/(2B) sum_i [sp(a_i) + sp(-b_i)]
 * The gradient is the full derivative, the two means included: with A_i = dL/da_i and Bv_i = dL/db_i,
 *   d_real_i = grad_scale (A_i - mean(Bv))      d_fake_i = grad_scale (Bv_i - mean(A)).
 * Everything in double up to the fp32 stores; sums in a fixed order; one launch of one block; no atomics; any B >= 1.
 * d_real or d_fake may be NULL (the generator's step detaches the real logits).  `workspace` is not used and may be NULL
 * (the argument keeps the calling convention of the other loss kernels).
 * srk_ragan_loss_host: the same formulas (ragan_common.h) on host pointers, results in double; d_real / d_fake may be NULL. */
int srk_ragan_loss_forward_backward(const float* real, const float* fake, int B, int for_generator, float grad_scale,
                                    float* loss, float* d_real, float* d_fake, void* workspace, void* stream);
int srk_ragan_loss_host(const float* real, const float* fake, int B, int for_generator, double grad_scale, double* loss,
                        double* d_real, double* d_fake);

/* ---- Shifted-window self-attention: SwinIR's attention operator (csrc/wattn.hip, csrc/wattn_common.h) ----------------
 * (Additive again: new entry points only, srk_version() and everything existing unchanged.)
 * qkv dense NHWC [N][H][W][3C], the qkv projection with its bias applied, channels q | k | v, each split heads x d
 * (d = C / heads); table [(2 window - 1)^2][heads]; out, dout [N][H][W][C]; dqkv as qkv.
 * The map is rolled by -shift along both axes and cut into window x window windows of T = window^2 tokens.  Per window
 * and head, with i, j tokens in row-major order:
 *   S = d^-0.5 Q K^T + table[rel(i, j)][head] + mask(i, j)      P = softmax_j S      O = P V
 *   rel(i, j) = (y_i - y_j + window - 1) (2 window - 1) + (x_i - x_j + window - 1)
 *   mask(i, j) = -100 where shift > 0 and the tokens' region ids differ; a token at shifted (r, c) has id
 *   3 band(r, H) + band(c, W), band(r, H) = 0 if r < H - window, 1 if r < H - shift, else 2
 * and O is written where the token was read (the roll back).  Neither mask nor index exists in memory.  From dout:
 *   dV = P^T dO   dP = dO V^T   dS = P (dP - rowsum(P dP))   dQ = d^-0.5 dS K   dK = d^-0.5 dS^T Q
 *   dtable[r][head] = sum over N, windows and pairs with rel(i, j) = r of dS
 * fp32 FMAs; one wave a (window, head), one lane a token.  dtable goes through per-block bins added up in a fixed order;
 * the grid is a function of the shape.  No atomics: two calls on the same inputs give the same bits.
 * Supported (SRK_ERR_BAD_ARG otherwise, the message names the number): 2 <= window <= 8, 0 <= shift < window, H and W
 * multiples of window, heads dividing C, d <= SRK_WATTN_MAX_HEAD_DIM.
 * srk_window_attention_forward: lse [N * (H / window) * (W / window)][heads][64], the row log-sum-exp the backward
 *   reads, or NULL when no backward follows.
 * srk_window_attention_backward: reads the forward's out and lse.  dtable == NULL: no table gradient (and no workspace);
 *   else dtable = beta * dtable + gradient (beta == 0 never reads it) through srk_window_attention_workspace() bytes.
 * srk_window_attention_host: the definition in double on host pointers, from the loop of wattn_common.h.  dout == NULL:
 *   forward only.  srk_window_attention_region / _rel_index / _token_pixel: the header's index functions (-1 for
 *   arguments out of range); region takes SHIFTED coordinates, token_pixel returns y * W + x of the unshifted map. */
#define SRK_WATTN_MAX_HEAD_DIM 32
size_t srk_window_attention_workspace(int N, int H, int W, int C, int heads, int window);
int srk_window_attention_forward(const float* qkv, const float* table, int N, int H, int W, int C, int heads, int window,
                                 int shift, float* out, float* lse, void* stream);
int srk_window_attention_backward(const float* dout, const float* qkv, const float* table, const float* out,
                                  const float* lse, int N, int H, int W, int C, int heads, int window, int shift,
                                  float* dqkv, float* dtable, float beta, void* workspace, size_t workspace_bytes,
                                  void* stream);
int srk_window_attention_host(const float* qkv, const float* table, const float* dout, int N, int H, int W, int C,
                              int heads, int window, int shift, double* out, double* dqkv, double* dtable);
int srk_window_attention_region(int H, int W, int window, int shift, int r, int c);
int srk_window_attention_rel_index(int window, int ti, int tj);
int64_t srk_window_attention_token_pixel(int H, int W, int window, int shift, int wy, int wx, int t);

/* ---- LayerNorm over the last axis with an affine, and the exact GELU (csrc/swin_pointwise.hip) ----------------------
 * x, y, dy, dx [rows][C] dense; gamma, beta [C]; mean, rstd [rows] (biased variance, rstd = 1 / sqrt(var + eps)).
 *   y = (x - mean) rstd gamma + beta        dx = rstd (g dy - mean_c(g dy) - xhat mean_c(g dy xhat)), xhat = (x - mean) rstd
 *   dgamma = sum_rows dy xhat               dbeta = sum_rows dy
 * Any C >= 1.  mean and rstd: both or neither (NULL: inference).  The parameter gradients go through
 * srk_layer_norm_workspace() bytes of per-range partials added up in index order; out = acc * out + gradient
 * (acc == 0 never reads out); either may be NULL, dx may be NULL.  No atomics.
 * GELU: y = x Phi(x) with erf; dx = dy (Phi(x) + x phi(x)) from the saved input.  16-byte accesses with a scalar tail
 * where every pointer is 16-byte aligned, else 4-byte accesses. */
size_t srk_layer_norm_workspace(int64_t rows, int C);
int srk_layer_norm_forward(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                           int64_t rows, int C, float eps, void* stream);
int srk_layer_norm_backward(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                            float* dx, float* dgamma, float* dbeta, float acc, int64_t rows, int C, void* workspace,
                            size_t workspace_bytes, void* stream);
int srk_gelu_forward(const float* x, float* y, size_t n, void* stream);
int srk_gelu_backward(const float* dy, const float* x, float* dx, size_t n, void* stream);

/* ---- Spectral normalisation of filters: Real-ESRGAN's U-Net discriminator (csrc/spectral_norm.hip) -------------------
 * (Additive again: new entry points only, srk_version() and everything existing unchanged.)
 * torch.nn.utils.spectral_norm(conv, n_power_iterations=1, eps, dim=0).  W is the dense [R][K] view of a filter, R = out
 * channels, K = in * kh * kw; u [R] and v [K] are the fp32 buffers of the power iteration.
 *   training:  v <- W^T u / max(||W^T u||, eps)   u <- W v / max(||W v||, eps)   (both written back in place)
 *   then       sigma = u . (W v)                  w_sn = W / sigma
 *   eval:      no update; sigma from the stored u and v.
 *   backward:  u, v constants; with G = dL/dw_sn:  dW = (G - <G, w_sn> u v^T) / sigma.
 * `saved` (R + K + 1 floats, or NULL): the u, v and sigma of THIS forward, for its backward: two forwards between two
 * optimizer steps have different ones.  Every dot product and norm is a double sum in an order that is a function of the
 * shape alone, through per-block partials; no atomics; u, v and w_sn are stored fp32 and used as stored.
 * srk_spectral_norm_forward: n <= SRK_SPECTRAL_MAX_LAYERS layers in three launches (two in eval mode); K <= 16384;
 *   workspace of srk_spectral_norm_workspace(layers, n) bytes, 8-byte aligned.
 * srk_spectral_norm_backward: one layer in two launches; dW = beta * dW + gradient (beta == 0 never reads dW); workspace of
 *   srk_spectral_norm_backward_workspace(R, K) bytes, 8-byte aligned.
 * 16-byte accesses along K where K % 4 == 0 and the pointers are 16-byte aligned, else 4-byte accesses.
 * srk_spectral_norm_host: one layer on host pointers from the same formulas (spectral_norm_common.h), u / v / results in
 *   double; u and v are updated in place in training mode; G and dW come together or are both NULL. */
#define SRK_SPECTRAL_MAX_LAYERS 16
typedef struct srk_spectral_layer {
  const float* W;            /* [R][K] */
  float* u;                  /* [R] */
  float* v;                  /* [K] */
  float* w_sn;               /* [R][K] out */
  float* saved;              /* [R + K + 1] out: u, v, sigma of this forward; or NULL */
  int32_t R, K;
} srk_spectral_layer;
size_t srk_spectral_norm_workspace(const srk_spectral_layer* layers, int n);
int srk_spectral_norm_forward(const srk_spectral_layer* layers, int n, int training, double eps, void* workspace,
                              size_t workspace_bytes, void* stream);
size_t srk_spectral_norm_backward_workspace(int R, int K);
int srk_spectral_norm_backward(const float* G, const float* w_sn, const float* saved, int R, int K, float* dW, float beta,
                               void* workspace, size_t workspace_bytes, void* stream);
int srk_spectral_norm_host(const float* W, int R, int K, int training, double eps, double* u, double* v, double* w_sn,
                           double* sigma, const double* G, double* dW);

/* ---- Bilinear x2 upsampling with a fused skip addition (csrc/bilinear.hip, csrc/bilinear_common.h) -------------------
 * y = F.interpolate(x + add, scale_factor=2, mode='bilinear', align_corners=False) on dense NHWC: x, add [N][H][W][C]
 * (add may be NULL), y [N][2H][2W][C].  Per axis of n inputs: output 2k reads (k - 1, k) with weights (0.25, 0.75), index 0
 * alone for k = 0; output 2k + 1 reads (k, min(k + 1, n - 1)) with (0.75, 0.25).
 * backward: dx = the adjoint applied to dy, in gather form: every dx element is written once and adds its at most 4 x 4
 * outputs in index order; no atomics.  dx is the gradient of x and of add alike.
 * 16-byte accesses along C where C % 4 == 0 and the pointers are 16-byte aligned, else 4-byte accesses.
 * srk_upsample_bilinear2x_host: both halves in double on host pointers; x and y, dy and dx come in pairs, a NULL pair is skipped. */
int srk_upsample_bilinear2x_forward(const float* x, const float* add, float* y, int N, int H, int W, int C, void* stream);
int srk_upsample_bilinear2x_backward(const float* dy, float* dx, int N, int H, int W, int C, void* stream);
int srk_upsample_bilinear2x_host(const float* x, const float* add, const float* dy, int N, int H, int W, int C, double* y,
                                 double* dx);

/* ---- Vanilla GAN loss on logits (csrc/gan_logit.hip, csrc/ragan_common.h) --------------------------------------------
 * n >= 1 logits of any shape, dense.  sp(x) = max(x, 0) + log1p(exp(-|x|)):
 *   target_is_real != 0   L = mean sp(-x)      d_logits = grad_scale * -sigmoid(-x) / n
 *   target_is_real == 0   L = mean sp(x)       d_logits = grad_scale * sigmoid(x) / n
 * One pass writes the gradient and per-block double partials (the grid is a function of n), one block finishes them in a
 * fixed order; no atomics.  d_logits may be NULL.  workspace: srk_gan_logit_loss_workspace_bytes() bytes, 8-byte aligned.
 * srk_gan_logit_loss_host: the same formulas on host pointers, results in double. */
size_t srk_gan_logit_loss_workspace_bytes(void);
int srk_gan_logit_loss_forward_backward(const float* logits, size_t n, int target_is_real, float grad_scale, float* loss,
                                        float* d_logits, void* workspace, void* stream);
int srk_gan_logit_loss_host(const float* logits, size_t n, int target_is_real, double grad_scale, double* loss,
                            double* d_logits);

/* ---- The multi-layer VGG feature loss: one tapped layer, fused (csrc/vgg_tap.hip, csrc/vgg_tap_common.h) ---------------
 * (Additive again: new entry points and one enum, srk_version() and everything existing unchanged.)
 * a (the prediction's map, takes the gradient) and b (the target's) are the PRE-activation maps of one VGG layer, dense
 * NHWC [N][H][W][C] fp32; weight >= 0.  The tap's term is weight * mean |a - b| over all N*H*W*C elements; `mode` says
 * what the head runs behind the tap, and the tap runs it:
 *   SRK_VGG_TAP_POOL   ReLU, MaxPool 2 x 2     forward writes ya = pool(relu(a)), yb = pool(relu(b))  [N][H/2][W/2][C]
 *                                              backward  da = c * sign(a - b) + route(g)       g: the gradient of ya
 *   SRK_VGG_TAP_RELU   ReLU, then a conv       forward writes ya = relu(a), yb = relu(b)       [N][H][W][C]
 *                                              backward  da = c * sign(a - b) + (a > 0 ? g : 0)
 *   SRK_VGG_TAP_LAST   nothing                 forward writes no map (ya, yb, g are ignored)   da = c * sign(a - b)
 * sign(0) = 0.  route(g): the winner of a window is the first strictly greater value in (row, column) order, and a
 * window whose maximum is <= 0 routes nothing -- srk_maxpool2x2_backward with relu_input = 1.  The windows are
 * ceil(H/2) x ceil(W/2): with odd H or W the trailing row / column counts in the term and gets its da, and has no pooled
 * output (floor mode).  POOL needs H, W >= 2.
 * One launch each way.  Every element of ya, yb and da is written exactly once: nothing is cleared, no atomics.
 * 16-byte accesses where C % 4 == 0 and every pointer is 16-byte aligned, else 4-byte accesses.
 * The term's sum: |a - b| with the difference in fp64, per-block fp64 partials in a fixed order.  The forward writes row
 * `row` of the workspace, srk_vgg_tap_workspace_bytes(rows) bytes, 8-byte aligned, all rows of which must be written by
 * taps before srk_vgg_tap_finish (one launch) adds them in index order into *loss (fp32) = sum_k weight_k * mean_k.  Two
 * runs on the same inputs give the same bits.
 * srk_vgg_tap_backward: c = weight * seed / (N*H*W*C) on the host; factor: NULL, or one fp32 on the device that multiplies
 *   c (an upstream gradient that is not the node's own seed).
 * srk_vgg_tap_plan: the blocks of either launch of that mode on the 16-byte (vec = 1) or 4-byte path and, in *items, the
 *   items its grid-stride loop walks (256 per block and pass); a negative status for bad sizes.
 * srk_vgg_tap_forward_host / _backward_host: the same window bodies on host pointers, in double up to the fp32 stores;
 *   *loss = weight * mean |a - b| in double; c as above (with any factor folded in). */
typedef enum srk_vgg_tap_mode { SRK_VGG_TAP_POOL = 0, SRK_VGG_TAP_RELU = 1, SRK_VGG_TAP_LAST = 2 } srk_vgg_tap_mode;
size_t srk_vgg_tap_workspace_bytes(int rows);
int srk_vgg_tap_plan(int N, int H, int W, int C, int mode, int vec, long long* items);
int srk_vgg_tap_forward(const float* a, const float* b, int N, int H, int W, int C, int mode, double weight, int row,
                        int rows, void* workspace, float* ya, float* yb, void* stream);
int srk_vgg_tap_finish(const void* workspace, int rows, float* loss, void* stream);
int srk_vgg_tap_backward(const float* a, const float* b, const float* g, int N, int H, int W, int C, int mode, double c,
                         const float* factor, float* da, void* stream);
int srk_vgg_tap_forward_host(const float* a, const float* b, int N, int H, int W, int C, int mode, double weight,
                             double* loss, float* ya, float* yb);
int srk_vgg_tap_backward_host(const float* a, const float* b, const float* g, int N, int H, int W, int C, int mode, double c,
                              float* da);

/* ---- NIQE features on the device (csrc/niqe.hip, csrc/niqe_common.h) ---------------------------------------
 * (Additive again: new entry points only, srk_version() and everything existing unchanged.)
 * NIQE (Mittal, Soundararajan, Bovik 2013) as BasicSR's calculate_niqe states it -- written down from memory of that code,
 * not checked against it; the yardstick is the numpy / scipy restatement in tests/niqe_ref.py.  The entry points make the
 * [blocks, 36] natural-scene-statistics features of one picture; the 36 x 36 finish is the caller's (ops.niqe_finish).
 * img: one picture [C, H, W], C in {1, 3}, read through element strides (c, h, w).  is_u8 == 0: fp32, each value quantised
 *   by the byte rule of srk_float_to_u8_image, (uint8)(clamp(v, 0, 1) * 255.0f); is_u8 != 0: bytes, taken as they are.
 * shave >= 0, block even in 8 .. 96.
 * 1. Luma.  C == 3: Y = rint(16 + (65.481 R + 128.553 G + 24.966 B) / 255) on the bytes, in double, ties to even (BT.601
 *    studio range; NOT the Pillow luma of SRK_SSIM_Y8).  C == 1: the byte.
 * 2. Crop.  shave pixels off each side, then the top-left nh*block x nw*block pixels, nh = (H - 2 shave) / block, nw
 *    likewise.  Nothing outside the crop is read again; every border rule below acts at the crop's edges.  nh * nw < 2 is
 *    SRK_ERR_BAD_ARG.
 * 3. Two scales s = 1, 2, block side b_s = block / s, on the plane P_s (P_1 = Y).  Window g[i] = exp(-(i - 3)^2 /
 *    (2 (7/6)^2)), i = 0 .. 6, normalised to sum 1, separable, plane borders replicated.  mu = G P, sigma = sqrt(|G P^2 -
 *    mu^2|), n = (P - mu) / (sigma + 1).
 * 4. Per block B (b_s x b_s of n) five maps: m_0 = B, m_k = B * roll(B, shift_k), shifts (0,1), (1,0), (1,1), (1,-1) over
 *    (rows, columns), circular INSIDE the block (numpy's roll).
 * 5. Per map over its M = b_s^2 values: c_neg, q_neg = count and sum of squares of the values < 0; c_pos, q_pos of the
 *    values > 0 (zeros belong to neither); a = sum |m|; q = sum m^2.
 * 6. AGGD fit per map: ls = sqrt(q_neg / c_neg), rs = sqrt(q_pos / c_pos), gh = ls / rs, rhat = (a / M)^2 / (q / M),
 *    rn = rhat (gh^3 + 1)(gh + 1) / (gh^2 + 1)^2, alpha = gam[argmin_j (r_gam[j] - rn)^2] (first index on a tie),
 *    gam[j] = 0.2 + 0.001 j, j < SRK_NIQE_TABLE, r_gam = Gamma(2/gam)^2 / (Gamma(1/gam) Gamma(3/gam)),
 *    beta_l = ls sqrt(Gamma(1/alpha) / Gamma(3/alpha)), beta_r likewise from rs.  c_neg == 0, c_pos == 0 or q == 0 makes
 *    every feature of that map NaN.
 * 7. 18 features per scale: [alpha_0, (beta_l0 + beta_r0) / 2], then per product map [alpha_k, (beta_rk - beta_lk)
 *    Gamma(2/alpha_k) / Gamma(1/alpha_k), beta_lk, beta_rk].  features[blk][0..17] scale 1, [18..35] scale 2 of the block
 *    at the same grid position, blk = by * nw + bx.
 * 8. P_2 = shrink(P_1): MATLAB's antialiased bicubic at exactly 1/2, in double: output i reads inputs 2i - 3 .. 2i + 4
 *    with the weights [-3, -9, 29, 111, 111, 29, -9, -3] / 256; out-of-range indices reflect with the edge sample
 *    repeated (-1 -> 0, -2 -> 1, n -> n - 1).  Bytes times these weights add exactly in double, so P_2 does not depend on
 *    the order of the two passes.  P_2 is not rounded.
 * 9. sharpness (may be NULL): [blocks], the mean of scale 1's sigma over the block.
 * tables: 3 * SRK_NIQE_TABLE doubles (srk_niqe_tables_host): r_gam, sqrt(Gamma(1/g) / Gamma(3/g)), Gamma(2/g) / Gamma(1/g);
 *   on the device for srk_niqe_features, on the host for srk_niqe_features_host.
 * workspace: srk_niqe_workspace_bytes(H, W, block) bytes, 8-byte aligned (holds P_2, fp64; 0 for bad sizes).
 * Two launches a picture; all arithmetic fp64; sums in a fixed order through per-thread, per-wave and per-block
 * partials, no atomics: two calls on the same inputs return the same bits.
 * srk_niqe_features_host: the same definition in plain C++ double on HOST pointers. */
enum { SRK_NIQE_TABLE = 9801, SRK_NIQE_FEATURES = 36 };
int srk_niqe_tables_host(double* out);
size_t srk_niqe_workspace_bytes(int H, int W, int block);
int srk_niqe_features(const void* img, int is_u8, const int64_t* strides, int C, int H, int W, int shave, int block,
                      const double* tables, double* features, double* sharpness, void* workspace, void* stream);
int srk_niqe_features_host(const void* img, int is_u8, const int64_t* strides, int C, int H, int W, int shave, int block,
                           const double* tables, double* features, double* sharpness);

/* ---- raw video frames (YUV4MPEG2 payloads) to the net and back (csrc/video.hip, csrc/video_common.h) ----------------
 * (Added without a change of srk_version(): new entry points only, nothing existing changed.)
 * A frame is planar and 8-bit: Y [H][W], then for SRK_YUV_420 Cb and Cr [H/2][W/2] (H and W even: an odd size is refused),
 * for SRK_YUV_444 Cb and Cr [H][W], for SRK_YUV_MONO nothing; all dense.  N frames lie frame_stride bytes apart
 * (>= the frame's bytes) and may start at any address.  Samples are full-range JFIF values; the colour conversions are
 * those of srk_ycc_to_rgb_u8 / srk_rgb_to_ycc_u8 (Pillow's tables), the quantisation srk_float_to_u8_image's.
 * srk_yuv_unpack: frames -> out, dense fp32 [N][C][H][W], one launch.
 *   C = 1: out = Y / 255.0f; the chroma is not read.
 *   C = 3: R, G, B / 255.0f from Y and full-resolution Cb / Cr: the frame's own planes (444), the constant 128 (mono), or
 *   chroma_full (420; dense 8-bit [2][N][H][W], all Cb planes then all Cr planes: what srk_img_resize_u8 makes of the
 *   frames' chroma planes in two calls with plane_stride = frame_stride).  chroma_full is not read otherwise.
 * srk_yuv_pack: x, fp32 [N][C][OH][OW] through four element strides (image, channel, row, pixel), -> N frames of OW x OH,
 *   one launch.  Every value is quantised as (uint8)(min(max(v, 0), 1) * 255.0f); NaN gives 0.
 *   C = 1: Y' = the quantised plane; chroma (dense 8-bit [2][N][ch][cw], ch x cw the frame's chroma size; not read for
 *   mono) is copied into the frames' Cb and Cr slots.
 *   C = 3: Y', Cb', Cr' from the quantised R, G, B.  444 writes all three, mono Y' only.  420 writes per 2 x 2 quad
 *   (a b / c d) of Cb' (and of Cr') the sample (((a + b + 1) >> 1) + ((c + d + 1) >> 1) + 1) >> 1, which is Pillow's
 *   resize((OW / 2, OH / 2), Image.BOX): it rounds after each pass, so this is not the four-sample mean.
 * SRK_ERR_BAD_ARG before anything is launched: null pointer, a size <= 0, C not 1 or 3, an unknown sub, an odd 420 size,
 *   frame_stride below the frame's bytes, negative strides, missing chroma planes.
 * The _host twins are the same definitions on HOST pointers (they compile the kernels' per-pixel header). */
enum { SRK_YUV_420 = 0, SRK_YUV_444 = 1, SRK_YUV_MONO = 2 };
int srk_yuv_unpack(const uint8_t* frames, int64_t frame_stride, int N, int H, int W, int sub, int C,
                   const uint8_t* chroma_full, float* out, void* stream);
int srk_yuv_pack(const float* x, const int64_t* strides, int N, int C, int OH, int OW, int sub, const uint8_t* chroma,
                 uint8_t* frames, int64_t frame_stride, void* stream);
int srk_yuv_unpack_host(const uint8_t* frames, int64_t frame_stride, int N, int H, int W, int sub, int C,
                        const uint8_t* chroma_full, float* out);
int srk_yuv_pack_host(const float* x, const int64_t* strides, int N, int C, int OH, int OW, int sub, const uint8_t* chroma,
                      uint8_t* frames, int64_t frame_stride);

#ifdef __cplusplus
}
#endif
#endif /* SRK_H_ */
