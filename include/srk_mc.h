#ifndef SRK_MC_H_
#define SRK_MC_H_
/* libsrk's motion-compensation entry points (VESPCN).  Status codes, conventions and the error slot are include/srk.h's. */
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- motion compensation: flow warp, early fusion and the flow-smoothness term (csrc/mc.hip, csrc/mc_common.h) ----
 * An extension header of its own: include/srk.h, its symbol list and srk_version() are unchanged.  The binding reads this
 * file with the same reader (_header.py) and binds its functions beside srk.h's (_lib.py).  DESIGN.md 38.
 * Everything is in PIXEL coordinates.  A flow is [.., 2, H, W] fp32 read through four element strides (any dense layout):
 * channel 0 the x displacement, channel 1 the y displacement.
 * warp(img, flow)[n, c, y, x]: xs = x + flow_x, ys = y + flow_y, each clamped to [0, W-1] / [0, H-1] (a NaN goes to 0);
 *   x0 = floor(xs), x1 = min(x0 + 1, W-1), wx = xs - x0, the same in y, then the bilinear value of the four corners:
 *   F.grid_sample(mode='bilinear', padding_mode='border', align_corners=True) on pixel coordinates.
 *   d/dflow_x = ((v01 - v00)(1 - wy) + (v11 - v10) wy) * [0 < unclamped xs < W-1], symmetric in y: on an integer
 *   coordinate the right-hand cell's slope.  The image takes no gradient (its adjoint would be a scatter).
 * srk_motion_fuse_forward: frames [N,3,C,H,W] dense (t-1, t, t+1), flow [2N,2,H,W] (rows 0..N-1 move t-1 onto t, rows
 *   N..2N-1 move t+1 onto t) -> fused, dense NHWC [N,H,W,3C] = [warp(t-1) | frame t | warp(t+1)], and *mc_loss = the mean
 *   over all 2 N C H W elements of (warped - frame t)^2.  One pass (a thread a pixel) and a one-block finish of the
 *   per-block fp64 partials in a fixed order.  workspace: srk_mc_workspace_bytes() bytes, 8-byte aligned.
 * srk_motion_fuse_backward: one launch, dflow = sum_c (g_fused_c + s (warped_c - cur_c)) d warp_c / d flow with
 *   s = seed * 2 / (2 N C H W), times *seed_dev where seed_dev (a device scalar) is not NULL.  The samples are recomputed
 *   from frames; g_fused ([N,3C,H,W] through four element strides) may be NULL (= 0).  dflow [2N,2,H,W] through its own
 *   strides; every element is written once.
 * srk_flow_warp_forward / _backward: the same bodies for one image [N,C,H,W] (through strides) and one flow [N,2,H,W]:
 *   out dense NHWC [N,H,W,C]; dflow = sum_c g_c d warp_c / d flow.
 * srk_flow_huber_forward_backward: flow [M,2,H,W]; forward differences dx, dy of both components (0 at the last column
 *   and row), h = sqrt(eps + dx_u^2 + dy_u^2 + dx_v^2 + dy_v^2) per pixel, *loss = mean over M H W; dflow (may be NULL;
 *   stored with the flow's strides) = grad_scale * d loss / d flow, a gather over p, p - ex, p - ey.  One pass and the
 *   finish; fp64 up to the fp32 stores.  eps > 0.  workspace as above.
 * No atomics anywhere: two calls on the same inputs return the same bits.
 * The _host twins compile the same per-pixel header in double on HOST pointers: fused / out / g / dflow are dense NCHW
 *   doubles, dflow and g may be NULL; srk_motion_fuse_host folds `seed` as the backward above does. */
size_t srk_mc_workspace_bytes(void);
int srk_motion_fuse_forward(const float* frames, const float* flow, const int64_t* flow_strides, int N, int C, int H, int W,
                            float* fused, float* mc_loss, void* workspace, void* stream);
int srk_motion_fuse_backward(const float* frames, const float* flow, const int64_t* flow_strides, const float* g_fused,
                             const int64_t* g_strides, int N, int C, int H, int W, float seed, const float* seed_dev,
                             float* dflow, const int64_t* dflow_strides, void* stream);
int srk_flow_warp_forward(const float* img, const int64_t* img_strides, const float* flow, const int64_t* flow_strides, int N,
                          int C, int H, int W, float* out, void* stream);
int srk_flow_warp_backward(const float* img, const int64_t* img_strides, const float* flow, const int64_t* flow_strides,
                           const float* g, const int64_t* g_strides, int N, int C, int H, int W, float* dflow,
                           const int64_t* dflow_strides, void* stream);
int srk_flow_huber_forward_backward(const float* flow, const int64_t* flow_strides, int M, int H, int W, float eps,
                                    float grad_scale, float* loss, float* dflow, void* workspace, void* stream);
int srk_motion_fuse_host(const float* frames, const float* flow, const int64_t* flow_strides, int N, int C, int H, int W,
                         double seed, const double* g_fused, double* fused, double* mc_loss, double* dflow);
int srk_flow_warp_host(const float* img, const int64_t* img_strides, const float* flow, const int64_t* flow_strides, int N,
                       int C, int H, int W, const double* g, double* out, double* dflow);
int srk_flow_huber_host(const float* flow, const int64_t* flow_strides, int M, int H, int W, double eps, double grad_scale,
                        double* loss, double* dflow);

#ifdef __cplusplus
}
#endif
#endif /* SRK_MC_H_ */
