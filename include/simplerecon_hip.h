/*
 * simplerecon_hip.h -- C ABI of libsimplerecon_hip.so (MI355X / gfx950).
 *
 * The upstream reference (nianticlabs/simplerecon) has NO native code and NO FFI:
 * its "plugin point" for this path is a Python class contract plus an attribute
 * swap (`model.cost_volume = model.cost_volume.to_fast()`, reference test.py:196-198).
 * This header is therefore the boundary a maintainer binds from Python (ctypes stub
 * in INTEGRATION.md); each entry point cites the reference code it replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to fp32 unless stated; tensors are dense in the
 *    stated layout; the caller owns and allocates every buffer (no allocation, no
 *    ownership transfer, no global mutable state, no host synchronisation inside);
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *  - return value: 0 = ok, SR_ERR_* for argument errors, 1000 + hipError_t for a
 *    failed launch.  Nothing throws across the ABI.  Re-entrant; safe from several
 *    host threads on different streams as long as workspaces are not shared.
 *  - 4x4 matrices are row-major, 16 floats.
 */
#ifndef SIMPLERECON_HIP_H_
#define SIMPLERECON_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SR_OK 0
#define SR_ERR_INVALID_ARGUMENT 1
#define SR_ERR_UNSUPPORTED 2
#define SR_ERR_WORKSPACE_TOO_SMALL 3
#define SR_ERR_HIP_BASE 1000

/* ---- run-time switches (r05) ----------------------------------------------------------------------------------------
 * Every tuning / ablation switch of the library, and the two fenced split-precision modes (which change the numerics of the
 * calls that honour them), is an entry of ONE option table: read atomically by the entry points, set explicitly with
 * sr_option_set().  An entry is initialised once, at the library's first option access, from the environment variable of the
 * same name (tuning runs: `SR_WINO_XCD=0 python ...`); after that the environment is never read again -- no getenv() on any
 * launch path, no setenv() by any host.  The table is PROCESS-WIDE: a value set while another thread is launching applies to
 * that thread's next launch, and a HIP graph captured under a mode keeps the kernels of that mode.  Integer options take the
 * integer; the split modes take 0 = off (fp32 MFMA: the product path), 1 = bf16 pieces, 2 = f16 pieces (-1 = the unknown
 * string an environment variable held: the entry points that honour the mode return SR_ERR_INVALID_ARGUMENT); SR_MLP_TILE
 * takes the codes listed at sr_mlp_volume_tile_shape (environment: auto, flat, 2x32, 4x16, 8x8; -1 as above).
 * The two split modes differ in who reads them.  SR_OPT_MLP_SPLIT is read by the MLP entry points, once per call: the pack
 * and the sweep inside one sr_mlp_volume_fwd see one value whatever another thread sets meanwhile.  SR_OPT_WINO_SPLIT is the
 * switch a HOST reads to choose the `split_format` argument of sr_wino_pack_weights and sr_conv3x3_wino_splitk_nhwc_fwd: a
 * packed Winograd weight outlives the call that made it, so its format travels with it as a value, and the library's
 * Winograd launchers do not consult the option. */
enum {
  SR_OPT_MLP_SPLIT = 0, SR_OPT_WINO_SPLIT, SR_OPT_WINO_XCD, SR_OPT_WINO_NT, SR_OPT_WINO_KSPLIT, SR_OPT_CONV_WINO,
  SR_OPT_CONV_TILE, SR_OPT_CONV_KSPLIT, SR_OPT_PW_NT, SR_OPT_PW_KS, SR_OPT_PT_CFG, SR_OPT_PT_KS, SR_OPT_DOT_LDS,
  SR_OPT_DOT_LDS_G, SR_OPT_DOT_LDS_CULL, SR_OPT_DOT_LDS_CAP, SR_OPT_UPSAMPLE_QUAD, SR_OPT_POOL_STREAM,
  SR_OPT_MLP_TILE,
  SR_OPT_COUNT
};
int sr_option_count(void);
const char* sr_option_name(int id);               /* = the environment variable that seeds it, e.g. "SR_WINO_XCD" */
int sr_option_id(const char* name);               /* -1: no such option */
int sr_option_get(int id, int* value);
int sr_option_set(int id, int value, int* previous /* may be NULL */);
int sr_option_default(int id, int* value);

/* ABI version; bumped on any signature change. */
int sr_abi_version(void);

/* Name of the GPU architecture this library was compiled for ("gfx950"). */
const char* sr_target_arch(void);

/* ------------------------------------------------------------------ cost volume --
 *
 * Depth planes are addressed  planes[b*ps_b + j*ps_d + y*ps_y + x*ps_x]  (strides in
 * elements): (D,1,0,0) for the [B,D] values of generate_depth_planes (reference
 * modules/cost_volume.py:100-136), (D*h*w, h*w, w, 1) for a caller-supplied
 * depth_planes_bdhw (cost_volume.py:247, 297-299).
 *
 * The volume is written at  out_cv[b*cv_sb + j*cv_sd + (y*w + x)*cv_sp]:
 * (D*h*w, h*w, 1) = the reference's b,d,h,w layout, (D*h*w, 1, D) = channels-last.
 */

/* Scratch bytes needed by sr_dot_volume_fwd / sr_mlp_volume_fwd for these sizes. */
size_t sr_volume_workspace_bytes(int B, int K, int C, int h, int w);

/* Stage 1 of either sweep: per-(b,k) geometry records (P = K_src @ T_src_cur, reference
 * utils/geometry_utils.py:78; source camera centres and the DVMVS pose measures of
 * geometry_utils.py:178-191 when T_cur_src != NULL) and the channels-last repack of `src`
 * ([B,K,C,h,w] -> [B*K, h*w, C]) into `workspace`.  T_cur_src = cur_cam_T_src_cam ("src_poses"),
 * [B,K,16], may be NULL for the dot model. */
int sr_volume_prepare(const float* src, const float* K_src, const float* T_src_cur,
                      const float* T_cur_src, int B, int K, int C, int h, int w, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Stage 2 of the dot model: the sweep kernel alone, on a workspace filled by
 * sr_volume_prepare for the same sizes (lets a caller time / profile / re-run it alone). */
int sr_dot_volume_sweep(const float* cur, const float* invK_cur, const float* planes, int64_t ps_b,
                        int64_t ps_d, int64_t ps_y, int64_t ps_x, int B, int K, int C, int h, int w,
                        int D, float* out_cv, int64_t cv_sb, int64_t cv_sd, int64_t cv_sp,
                        float* out_lowest, uint8_t* out_mask, void* workspace,
                        size_t workspace_bytes, void* stream);

/* Pointwise (1x1, stride 1) convolution as a hand-written fp32-MFMA GEMM (csrc/sr_pw.hip), deterministic:
 *   out[b,p,co] = act( sum_ci gate[b,ci] * in[b,p,ci] * W[co,ci] + bias[co] + residual[b,p,co] ),  p = 0 .. HW-1
 * on channels-last views (batch stride, pixel stride in floats; channel slices of wider buffers are fine).  `packed_w` comes
 * from sr_conv_pack_weights(ksize = 1) (eval-mode BatchNorm folded by the caller); `gate` ([B][Cin], may be null) is the
 * squeeze-excite gate of an MBConv block, applied to the A operand while it is loaded; `residual` may be null; `act_code`
 * as `leaky_slope` of sr_conv2d_nhwc_fwd.  Replaces BasicBlock's 1x1 skip convolution (reference modules/layers.py:20-22,
 * 57-62) and nn.Conv2d(k=1) + BatchNorm (+ SiLU) (+ squeeze-excite scaling of the input) of the image-prior encoder's
 * MBConv blocks (reference experiment_modules/depth_model.py:110-116).  Needs Cin % 4 == 0 and 16-byte aligned input rows
 * (sr_pw_conv_supported; SR_ERR_UNSUPPORTED otherwise -> sr_conv2d_nhwc_fwd).  sr_pw_conv_plan reports the launch plan
 * (32-channel tiles per wave, K split across the waves of a workgroup) chosen for a shape. */
/* 16-bit activation I/O (training under torch.autocast; reference options.py:100-101 `precision: 16`, train.py:132): the
 * same two operators on fp16 (io_dtype = 1) / bf16 (io_dtype = 2) input / residual / output tensors (strides in ELEMENTS;
 * four channels = one 8-byte access, 8-byte aligned rows), widened to fp32 on load and rounded to nearest even on store;
 * weights (packed as for the fp32 entry points), bias, transforms and the MFMA accumulation stay fp32.  The result equals the
 * fp32 entry point's result on the widened inputs, rounded once.  io_dtype = 0 forwards to the fp32 entry point.  The
 * Winograd form never splits K; the pointwise form takes no gate. */
int sr_conv3x3_wino_io_nhwc_fwd(const void* in, int64_t in_batch_stride, int in_pix_stride, const float* packed_u,
                                const float* bias, const void* residual, int64_t res_batch_stride, int res_pix_stride,
                                void* out, int64_t out_batch_stride, int out_pix_stride, int B, int H, int W, int Cin,
                                int Cout, float leaky_slope, int io_dtype, void* stream);
int sr_pw_conv_io_nhwc_fwd(const void* in, int64_t in_batch_stride, int in_pix_stride, const float* packed_w,
                           const float* bias, const void* residual, int64_t res_batch_stride, int res_pix_stride, void* out,
                           int64_t out_batch_stride, int out_pix_stride, int B, int HW, int Cin, int Cout, float act_code,
                           int io_dtype, void* stream);

/* LDS-tiled form of the same operator for BATCH-DENSE views (batch stride = HW * pixel stride, so the M = B * HW pixel rows
 * are one strided matrix): a workgroup stages (64 | 128) x 32 input and 32 x (64 | 128 | 160) weight tiles through LDS,
 * double-buffered -- each operand byte crosses the CU's vector-memory path once per workgroup instead of once per wave,
 * which is what the MBConv expand / project GEMMs of the image-prior encoder (M = 2 400 ... 9 600) need.  Small problems
 * split K across workgroups: raw partial tiles go to `workspace` (sr_pw_conv_tiled_workspace_bytes; may be null: no
 * split) and are added in index order (deterministic).  Same arguments otherwise; sr_pw_conv_tiled_plan reports the tile
 * configuration (0: 64x128, 1: 128x160, 2: 128x64, 3: 64x64) and the K split chosen for a shape. */
size_t sr_pw_conv_tiled_workspace_bytes(int M, int Cin, int Cout);
int sr_pw_conv_tiled_plan(int M, int Cin, int Cout, int can_split, int* cfg, int* ks);
int sr_pw_conv_tiled_nhwc_fwd(const float* in, int in_pix_stride, const float* packed_w, const float* bias,
                              const float* gate, const float* residual, int res_pix_stride, float* out,
                              int out_pix_stride, int M, int HW, int Cin, int Cout, float act_code, void* workspace,
                              size_t workspace_bytes, void* stream);
int sr_pw_conv_supported(int Cin, int Cout);
int sr_pw_conv_plan(int B, int HW, int Cin, int Cout, int* nt, int* ks);
int sr_pw_conv_nhwc_fwd(const float* in, int64_t in_batch_stride, int in_pix_stride, const float* packed_w,
                        const float* bias, const float* gate, const float* residual, int64_t res_batch_stride,
                        int res_pix_stride, float* out, int64_t out_batch_stride, int out_pix_stride, int B, int HW,
                        int Cin, int Cout, float act_code, void* stream);

/* Standalone forms of the reference's small geometry helpers (utils/geometry_utils.py) for callers outside the fused
 * sweeps; same operation order as the sweeps' internal arithmetic (FP contraction off).
 *  sr_backproject_fwd   BackprojectDepth.forward (:51-59): depth [B,h*w], invK [B,16] -> points [B,4,h*w]
 *  sr_project3d_fwd     Project3D.forward (:72-89): points [B,4,N], K [B,16], T = cam_T_world [B,16] -> [B,3,N]
 *                       (pixel x, pixel y, depth + eps)
 *  sr_pose_distance_fwd pose_distance (:178-191): T [n,16] -> [n,3] = (combined, R_measure, t_measure)
 *  sr_camera_rays_fwd   get_camera_rays (:143-175): points [B,3,N], T [B,16] (world_T_cam, or cam_T_world when
 *                       in_camera_frame) -> unit rays [B,3,N] */
int sr_backproject_fwd(const float* depth, const float* invK, float* out_points, int B, int h, int w, void* stream);
int sr_project3d_fwd(const float* points, const float* K, const float* T, float* out, int B, int N, float eps,
                     void* stream);
/* Adjoints for the training losses that call the two modules (reference losses.py via geometry_utils.py:51-59, 72-89):
 * d_depth [B,h*w] from d_points [B,4,h*w]; d_points [B,4,N] from d_out [B,3,N].  Intrinsics / poses are data. */
int sr_backproject_bwd(const float* grad_points, const float* invK, float* grad_depth, int B, int h, int w, void* stream);
int sr_project3d_bwd(const float* grad_out, const float* points, const float* K, const float* T, float* grad_points, int B,
                     int N, float eps, void* stream);
int sr_pose_distance_fwd(const float* T, float* out, int n, void* stream);
int sr_camera_rays_fwd(const float* points, const float* T, float* out, int B, int N, int in_camera_frame, void* stream);

/* Self-test of the LDS-staged sweep's packed reciprocal (csrc/sr_dot_volume_lds.hip): out_fast[i] = that reciprocal of
 * x[i], out_div[i] = the IEEE division 1.0f / x[i] every other kernel uses; they must agree bit for bit for
 * 2^-60 <= |x| <= 2^60 (outside that range the sweep itself takes the division).  No reference counterpart: the
 * reference divides in ATen (utils/geometry_utils.py:85). */
int sr_selftest_rcp(const float* x, float* out_fast, float* out_div, int n, void* stream);

/* Fused plane sweep of the dot-product model (= sr_volume_prepare + sr_dot_volume_sweep): replaces
 *   CostVolumeManager.build_cost_volume + forward      (cost_volume.py:237-380)
 *   = BackprojectDepth (utils/geometry_utils.py:51-59) + Project3D (:72-89)
 *   + F.grid_sample(bilinear, zeros, align_corners=False) (cost_volume.py:201-212)
 *   + sum_c(warped * cur) * (z' > 0), summed over views  (cost_volume.py:322-329)
 *   + argmax / gather of the depth planes               (cost_volume.py:338-342, 374-378)
 * in one launch per batch, never materialising the warped features.
 *
 *  cur        [B,C,h,w]      reference-frame matching features
 *  src        [B,K,C,h,w]    source-frame matching features
 *  K_src      [B,K,16]       source intrinsics at matching resolution (K_s1_b44)
 *  T_src_cur  [B,K,16]       src_cam_T_cur_cam  ("src_extrinsics")
 *  invK_cur   [B,16]         inverse reference intrinsics ("cur_invK")
 *  out_cv     see above;  out_lowest [B,h,w] (may be NULL);
 *  out_mask   [B,h,w] uint8 (may be NULL): any_k(z'>0) & any_k(2<u<w-2 & 2<v<h-2) at the
 *             LAST plane -- the rule of cost_volume.py:625-637 (the dot model itself
 *             returns None, cost_volume.py:286, 335).
 *  C must be a multiple of 4 and <= 32.
 */
int sr_dot_volume_fwd(const float* cur, const float* src, const float* K_src,
                      const float* T_src_cur, const float* invK_cur, const float* planes,
                      int64_t ps_b, int64_t ps_d, int64_t ps_y, int64_t ps_x, int B, int K, int C,
                      int h, int w, int D, float* out_cv, int64_t cv_sb, int64_t cv_sd,
                      int64_t cv_sp, float* out_lowest, uint8_t* out_mask, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Materialising front end of the sweeps, for the reference's public helper
 * CostVolumeManager.warp_features (cost_volume.py:139-234) / FastFeatureVolumeManager.warp_features
 * (:812-964): for Dp depth planes writes the back-projected points out_world [B,Dp,4,N] (may be NULL),
 * the source-camera depths z' out_depths [B,K,Dp,N], the bilinearly warped source features
 * out_warped [B,K,Dp,C,N], out_mask = (z' > 0) as float [B,K,Dp,N] and the sampling coordinates
 * out_pix [B,K,Dp,2,N] (may be NULL).  N = h*w.  B*K*Dp <= 65535. */
int sr_warp_features_fwd(const float* src, const float* K_src, const float* T_src_cur,
                         const float* invK_cur, const float* planes, int64_t ps_b, int64_t ps_d,
                         int64_t ps_y, int64_t ps_x, int B, int K, int C, int h, int w, int Dp,
                         float* out_world, float* out_depths, float* out_warped, float* out_mask,
                         float* out_pix, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------ metadata-MLP volume --
 *
 * Fused plane sweep of the hero model: replaces FeatureVolumeManager.build_cost_volume + forward
 * and FastFeatureVolumeManager (cost_volume.py:451-736, 967-1164, 345-380): per (b, d, y, x) the
 * C(1+K)+10K+4-channel vector of cost_volume.py:709-723 (warped source features, reference
 * features, masks, source depths, plane depth, dot products, ray angles, rays, pose measures) is
 * built in registers and pushed through MLP = Linear, LeakyReLU, Linear, LeakyReLU, Linear
 * (modules/networks.py:129-147, built at cost_volume.py:438) on fp32 MFMA.
 *
 *  T_cur_src  [B,K,16]  cur_cam_T_src_cam ("src_poses")
 *  W1 [hidden, Cin], b1 [hidden], W2 [hidden, hidden], b2 [hidden], W3 [1, hidden], b3 [1]
 *             = mlp.net.{0,2,4}.{weight,bias};  hidden must be 128, C must be 16.
 *  leaky_slope: 0.01 (nn.LeakyReLU default, networks.py:139); must lie in (0,1).
 *  out_mask as for the dot model (this model does return it, cost_volume.py:625-637).
 */
size_t sr_mlp_volume_workspace_bytes(int B, int K, int C, int h, int w, int hidden);

/* Packs the MLP parameters into the k-step order of the sweep kernel (into `workspace`).
 * Experiment switch (off by default; read once per call -- sr_mlp_volume_fwd hands its one reading to the pack and the
 * sweep inside it, a host that calls the pack and the sweep itself keeps the option still between the two): option
 * SR_MLP_SPLIT=bf16|f16 packs layers 1-2 as two 16-bit pieces per weight and selects the split-precision sweep kernel
 * (three exact 16-bit MFMA products per fp32 product, fp32 accumulate; K <= 7 source views, SR_ERR_UNSUPPORTED beyond;
 * unknown values: SR_ERR_INVALID_ARGUMENT).  Tensors handed in and results are fp32 either way. */
int sr_mlp_pack_weights(const float* W1, const float* b1, const float* W2, const float* b2,
                        const float* W3, const float* b3, int hidden, int B, int K, int C, int h, int w,
                        void* workspace, size_t workspace_bytes, void* stream);

/* The sweep kernel alone (whole chip), on a workspace filled by sr_volume_prepare (with T_cur_src) and
 * sr_mlp_pack_weights for the same sizes. */
int sr_mlp_volume_sweep(const float* cur, const float* invK_cur, const float* planes, int64_t ps_b,
                        int64_t ps_d, int64_t ps_y, int64_t ps_x, float leaky_slope, int B, int K,
                        int C, int h, int w, int D, float* out_cv, int64_t cv_sb, int64_t cv_sd,
                        int64_t cv_sp, float* out_lowest, uint8_t* out_mask, void* workspace,
                        size_t workspace_bytes, void* stream);

/* Which 64 pixels of the h x w map one wave of the sweep works on, under the current SR_MLP_TILE: a th x tw tile (th * tw =
 * 64; tiles row-major, lane l of tile (ty, tx) at y = ty*th + l / tw, x = tx*tw + l % tw, lanes past the image idle), or
 * th = 1, tw = 64 for 64 consecutive pixels of the flattened map.  A source view none of whose taps, over the wave's
 * pixels, lies inside the source image is skipped at that plane, and compact tiles are skipped more often than strips;
 * results do not depend on the shape, bit for bit.  Option SR_MLP_TILE (read per call): 0 "auto" (default) = the squarest of
 * 8x8, 4x16, 2x32 whose tile count is at most 1 % above ceil(h*w / 64), else the strip; 1 "flat" = the strip; 2 "2x32",
 * 3 "4x16", 4 "8x8" = that shape whatever it pads; anything else: SR_ERR_INVALID_ARGUMENT here and from the sweep. */
int sr_mlp_volume_tile_shape(int h, int w, int* th, int* tw);

/* = sr_volume_prepare + sr_mlp_pack_weights + sr_mlp_volume_sweep, with a CU reserve for this call:
 * reserve_cus = 0 runs the sweep on the whole chip; n > 0 makes its persistent grid leave n CUs to other streams, with the
 * plane chunk planned for the CUs that remain (results do not depend on it).  A reserve that would leave fewer than 8 CUs
 * means the whole chip; a negative one returns SR_ERR_INVALID_ARGUMENT. */
int sr_mlp_volume_fwd(const float* cur, const float* src, const float* K_src, const float* T_src_cur,
                      const float* T_cur_src, const float* invK_cur, const float* planes, int64_t ps_b,
                      int64_t ps_d, int64_t ps_y, int64_t ps_x, const float* W1, const float* b1,
                      const float* W2, const float* b2, const float* W3, const float* b3, int hidden,
                      float leaky_slope, int B, int K, int C, int h, int w, int D, float* out_cv,
                      int64_t cv_sb, int64_t cv_sd, int64_t cv_sp, float* out_lowest, uint8_t* out_mask,
                      int reserve_cus, void* workspace, size_t workspace_bytes, void* stream);

/* sr_mlp_volume_fwd for features that are channels-last already, read where they lie: cur [B, h*w, 16] and
 * src [B*K, h*w, 16], dense fp32 with 16-byte-aligned base addresses (SR_ERR_INVALID_ARGUMENT otherwise) -- the two slices
 * of the matching encoder's one output buffer.  No copy of either operand is made; geometry records, weight packing,
 * workspace size, every other argument and every bit of the results are those of sr_mlp_volume_fwd on the same features in
 * [B,16,h,w] / [B,K,16,h,w] order.  SR_ERR_UNSUPPORTED under SR_MLP_SPLIT (that kernel reads cur planar). */
int sr_mlp_volume_fwd_nhwc(const float* cur, const float* src, const float* K_src, const float* T_src_cur,
                           const float* T_cur_src, const float* invK_cur, const float* planes, int64_t ps_b,
                           int64_t ps_d, int64_t ps_y, int64_t ps_x, const float* W1, const float* b1,
                           const float* W2, const float* b2, const float* W3, const float* b3, int hidden,
                           float leaky_slope, int B, int K, int C, int h, int w, int D, float* out_cv,
                           int64_t cv_sb, int64_t cv_sd, int64_t cv_sp, float* out_lowest, uint8_t* out_mask,
                           int reserve_cus, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------- 2-D conv stack -------
 *
 * Channels-last activations: element (b, y, x, c) of a tensor lives at
 *   ptr[b*batch_stride + (y*W + x)*pix_stride + c]      (strides in elements),
 * so a channel slice of a wider concat buffer is addressed by offsetting `ptr` and keeping
 * the buffer's pix_stride -- producers write straight into the consumer's torch.cat layout
 * (reference modules/networks.py:83-89, 124).
 */

/* Floats needed for the packed form of a [Cout, Cin, k, k] Conv2d weight (k = 1 or 3). */
size_t sr_conv_packed_weight_floats(int Cout, int Cin, int ksize);

/* Packs an nn.Conv2d weight ([Cout,Cin,k,k], contiguous) into MFMA B-fragment order. */
int sr_conv_pack_weights(const float* weight, int Cout, int Cin, int ksize, float* packed, void* stream);

/* out = act( conv2d(in, W, stride, padding = k/2) + bias [+ residual] ), act = LeakyReLU(slope)
 * when leaky_slope >= 0, identity otherwise.  One launch replaces nn.Conv2d + bias + the
 * residual add + nn.LeakyReLU of BasicBlock.forward (reference modules/layers.py:68-85) and
 * conv3x3 / conv1x1 (layers.py:7-22).  ksize in {1,3}, stride in {1,2}; fp32 MFMA
 * (exact fp32 products and accumulation).  `residual` has the output's geometry. */
int sr_conv2d_nhwc_fwd(const float* in, int64_t in_batch_stride, int in_pix_stride,
                       const float* packed_weight, const float* bias, const float* residual,
                       int64_t res_batch_stride, int res_pix_stride, float* out,
                       int64_t out_batch_stride, int out_pix_stride, int B, int H, int W, int Cin,
                       int Cout, int ksize, int stride, float leaky_slope, void* stream);

/* Same operator with padding_mode="replicate" (border texels repeated instead of zeros): the 128 -> 16 conv of
 * the matching encoder's tail (reference modules/networks.py:191-197). */
int sr_conv2d_replicate_nhwc_fwd(const float* in, int64_t in_batch_stride, int in_pix_stride,
                                 const float* packed_weight, const float* bias, const float* residual,
                                 int64_t res_batch_stride, int res_pix_stride, float* out,
                                 int64_t out_batch_stride, int out_pix_stride, int B, int H, int W, int Cin,
                                 int Cout, int ksize, int stride, float leaky_slope, void* stream);

/* Same operator with explicit zero padding on each side (output size floor((H + top + bottom - ksize) / stride) + 1):
 * TensorFlow-"SAME" convolutions of the image-prior encoder pad 0 above / left and 1 below / right when a
 * stride-2 3x3 conv meets an even-sized map.  `leaky_slope` here -- and in every convolution entry point of this
 * header -- also carries the activation code: >= 0 LeakyReLU slope (0 = ReLU), SR_ACT_NONE = identity,
 * SR_ACT_SILU = x * sigmoid(x) (the Winograd entry points implement LeakyReLU / identity only). */
#define SR_ACT_NONE (-1.0f)
#define SR_ACT_SILU (-2.0f)
int sr_conv2d_padded_nhwc_fwd(const float* in, int64_t in_batch_stride, int in_pix_stride,
                              const float* packed_weight, const float* bias, const float* residual,
                              int64_t res_batch_stride, int res_pix_stride, float* out,
                              int64_t out_batch_stride, int out_pix_stride, int B, int H, int W, int Cin,
                              int Cout, int ksize, int stride, int pad_top, int pad_left, int pad_bottom,
                              int pad_right, float leaky_slope, void* stream);

/* sr_conv2d_nhwc_fwd with a split-K launch plan for 1x1 / stride-1 convolutions whose long input-channel chain would
 * otherwise run on a handful of workgroups (e.g. 1536 -> 256 channels on 8 x 15x20 pixels): the channel slabs of a
 * tile are spread over up to 8 work items that store raw partial sums into `workspace`, and a second launch adds them
 * in index order (deterministic) and applies bias / residual / activation.  sr_conv_splitk_workspace_bytes() returns
 * the workspace size for a shape, 0 when the plan would not split (then this entry point equals sr_conv2d_nhwc_fwd
 * and `workspace` may be NULL). */
size_t sr_conv_splitk_workspace_bytes(int B, int H, int W, int Cin, int Cout, int ksize, int stride);
int sr_conv2d_splitk_nhwc_fwd(const float* in, int64_t in_batch_stride, int in_pix_stride,
                              const float* packed_weight, const float* bias, const float* residual,
                              int64_t res_batch_stride, int res_pix_stride, float* out,
                              int64_t out_batch_stride, int out_pix_stride, int B, int H, int W, int Cin,
                              int Cout, int ksize, int stride, float leaky_slope, void* workspace,
                              size_t workspace_bytes, void* stream);

/* 3x3 / stride-1 / pad-1 convolution through Winograd F(2x2, 3x3) on the fp32 matrix cores: same operator and
 * epilogue as sr_conv2d_nhwc_fwd (fp32 products and accumulation; 2.25x fewer multiplies).  `packed_u` comes from
 * sr_wino_pack_weights (U = G g G^T in MFMA B-fragment order).  sr_conv_prefers_wino() tells whether this kernel
 * is expected to beat the direct one for a shape (enough 8x16-pixel regions, little padding). */
size_t sr_wino_packed_weight_floats(int Cout, int Cin);
/* `split_format` (fenced experiment): 0 = fp32 U, the product path; 1 = bf16 / 2 = f16 packs U as two 16-bit pieces (same
 * buffer size) for the split-precision kernel; anything else: SR_ERR_INVALID_ARGUMENT.  The format is a property of the
 * packed buffer: hand the same value to the sr_conv3x3_wino_splitk_nhwc_fwd calls that consume it.  Neither call reads
 * SR_OPT_WINO_SPLIT -- that option is where a host keeps its choice.  sr_conv3x3_wino_nhwc_fwd (and the 16-bit I/O form) are
 * the fp32-product entry points: they take format-0 weights and no longer follow the option. */
int sr_wino_pack_weights(const float* weight, int Cout, int Cin, int split_format, float* packed, void* stream);
int sr_conv_prefers_wino(int B, int H, int W, int Cin, int Cout, int ksize, int stride);
int sr_conv3x3_wino_nhwc_fwd(const float* in, int64_t in_batch_stride, int in_pix_stride,
                             const float* packed_u, const float* bias, const float* residual,
                             int64_t res_batch_stride, int res_pix_stride, float* out,
                             int64_t out_batch_stride, int out_pix_stride, int B, int H, int W, int Cin,
                             int Cout, float leaky_slope, void* stream);

/* The same operator through Winograd F(4x4, 3x3) (csrc/sr_wino4.hip, r05): 2.25 multiplies per output and channel pair
 * instead of F(2x2)'s 4 -- 1.78x fewer MFMAs on the full-resolution 64-channel layers of the UNet++ decoder (reference
 * modules/networks.py:20-96, BasicBlock modules/layers.py:24-85).  Interpolation points (0, +-1/2, +-2, inf): exact fp32
 * transforms, fp32 products and accumulation; fp32 error ~1.3e-6 of the output range on a 64-channel layer (F(2x2): 3e-7).
 * `packed_u` comes from sr_wino4_pack_weights (U = G g G^T, computed in double, in MFMA A-fragment order).  Needs channel
 * counts in whole quads and 16-byte aligned rows (SR_ERR_UNSUPPORTED otherwise: use sr_conv3x3_wino_nhwc_fwd).
 * sr_conv_prefers_wino4(): which kernel FORM is expected to beat F(2x2) for the shape -- 0 none, 1 two 4-wave workgroups per
 * CU, 3 one wave-specialised 8-wave workgroup per CU (pass it as `variant` of sr_conv3x3_wino4_variant_nhwc_fwd); `mode`
 * 0 = never, 1 = the rule fitted on profiles/r05_wino4_shape_sweep.txt, 2 = form 1 wherever the kernel applies.  The mode
 * is an ARGUMENT (the Python host reads SR_CONV_WINO4 once at import): no environment reads in here. */
size_t sr_wino4_packed_weight_floats(int Cout, int Cin);
int sr_wino4_pack_weights(const float* weight, int Cout, int Cin, float* packed, void* stream);
int sr_conv_prefers_wino4(int B, int H, int W, int Cin, int Cout, int mode);
int sr_conv3x3_wino4_nhwc_fwd(const float* in, int64_t in_batch_stride, int in_pix_stride, const float* packed_u,
                              const float* bias, const float* residual, int64_t res_batch_stride, int res_pix_stride,
                              float* out, int64_t out_batch_stride, int out_pix_stride, int B, int H, int W, int Cin,
                              int Cout, float leaky_slope, void* stream);

/* The same with the kernel form chosen by the caller: `variant` 0 = the default (what sr_conv3x3_wino4_nhwc_fwd launches),
 * 1 = two independent 4-wave workgroups per CU, 2 = one 8-wave workgroup per CU whose halves alternate transform and MFMA
 * phases (kept for A/B measurements).  Bit-identical results. */
int sr_conv3x3_wino4_variant_nhwc_fwd(const float* in, int64_t in_batch_stride, int in_pix_stride, const float* packed_u,
                                      const float* bias, const float* residual, int64_t res_batch_stride,
                                      int res_pix_stride, float* out, int64_t out_batch_stride, int out_pix_stride, int B,
                                      int H, int W, int Cin, int Cout, float leaky_slope, int variant, void* stream);

/* Split-K variant for layers with few output regions and a long chain of input slabs (deep low-resolution levels,
 * batch 1): work items cover Cin / ks input channels each and store raw partial outputs to `workspace`
 * ([ks][B, H*W, Cout] floats, 16-byte aligned); a second kernel adds them in index order (deterministic) and applies
 * bias + residual + LeakyReLU.  sr_wino_splitk_factor() = ks the launch plan picks for a shape (1: no split, no
 * workspace needed); with a NULL / too small workspace the call runs unsplit.  `split_format` = the format `packed_u` was
 * packed in (sr_wino_pack_weights); 1 / 2 select the split-precision kernel, which has the vector instantiation on fp32
 * tensors only (SR_ERR_UNSUPPORTED otherwise). */
int sr_wino_splitk_factor(int B, int H, int W, int Cin, int Cout);
size_t sr_wino_splitk_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int sr_conv3x3_wino_splitk_nhwc_fwd(const float* in, int64_t in_batch_stride, int in_pix_stride,
                                    const float* packed_u, const float* bias, const float* residual,
                                    int64_t res_batch_stride, int res_pix_stride, float* out,
                                    int64_t out_batch_stride, int out_pix_stride, int B, int H, int W, int Cin,
                                    int Cout, float leaky_slope, int split_format, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* The F(2x2) launch plan of a shape: output-channel block `nt` (32 nt channels per work item) and split-K factor `ks`
 * (either pointer may be NULL); `allow_split` = the launcher may split K (a usable workspace and the vector epilogue).  For
 * tests and sweeps: a launch reports what it ran through sr_last_launch. */
int sr_wino_conv_plan(int B, int H, int W, int Cin, int Cout, int allow_split, int* nt, int* ks);

/* ---- what a launch ran ----
 * The convolution launchers -- sr_conv2d_*_nhwc_fwd, sr_conv3x3_wino_*nhwc_fwd, sr_conv3x3_wino4_*nhwc_fwd, sr_pw_conv_*nhwc_fwd,
 * sr_pw_conv_tiled_nhwc_fwd, sr_stem7x7_fwd, sr_conv1x1_stats_nhwc_fwd, sr_conv3x3_c16_nhwc_fwd -- note, at the branch that
 * issues their main kernel, which instantiation that was and the padded problem it works through (a split-K finish or a pack
 * kernel beside it is not noted).  sr_last_launch() reports the calling thread's note: the kernel's name as a profiler shows
 * it, with the template arguments that were chosen per launch (`sr_wino_kernel<2, true, true>`, `sr_conv_kernel<3, 2, 1, 1, 8,
 * true>`, `sr_wino4pp_kernel`; the tiled pointwise kernel by its workgroup tile and K split: `sr_pw_tiled_kernel<64x128, ks 2,
 * false>`), and the FLOPs the kernel issues on that padded problem (2 per multiply-add; negative where none are counted: the
 * direct convolution kernels).  The note is valid ON THE CALLING THREAD UNTIL ITS NEXT LAUNCHER CALL, and only after a launcher
 * that returned SR_OK; reading it clears it, so SR_ERR_INVALID_ARGUMENT means no launcher has noted anything since the last
 * read (or a NULL / empty buffer).  `name` is cut to name_capacity - 1 characters; 64 hold every name.  Costs the launchers a
 * few thread-local integer stores; nothing is formatted before this call. */
int sr_last_launch(char* name, int name_capacity, double* executed_flops);

/* F.interpolate(scale_factor=2, mode="bilinear", align_corners=False) -- `upsample` of the
 * reference (utils/generic_utils.py:96-105) -- on channels-last data, [B,H,W,C] -> [B,2H,2W,C]. */
int sr_upsample2x_nhwc_fwd(const float* in, int64_t in_batch_stride, int in_pix_stride, float* out,
                           int64_t out_batch_stride, int out_pix_stride, int B, int H, int W, int C,
                           void* stream);

/* out[i] = exp(in[i]) over n contiguous floats: depth_pred = exp(log_depth_pred) (reference depth_model.py:392-400). */
int sr_exp_fwd(const float* in, float* out, int64_t n, void* stream);

/* ------------------------------------------------------ matching-feature encoder -------
 *
 * ResnetMatchingEncoder (reference modules/networks.py:149-205): antialiased ResNet-18 stem + layer1, then
 * conv1x1 -> InstanceNorm -> LeakyReLU(0.2) -> conv3x3 (replicate padding) -> InstanceNorm.  layer1 and the tail
 * convolutions go through sr_conv2d_nhwc_fwd / sr_conv3x3_wino_nhwc_fwd / sr_conv2d_replicate_nhwc_fwd with the
 * eval-mode BatchNorm folded into weight and bias by the caller; the entry points below cover the rest.
 */

/* Packed form of the stem weight nn.Conv2d(3, 64, 7, stride 2, padding 3, bias=False).weight ([64,3,7,7]);
 * only Cout = 64 is implemented (returns 0 / SR_ERR_UNSUPPORTED otherwise). */
size_t sr_stem_packed_weight_floats(int Cout);
int sr_stem_pack_weights(const float* weight, int Cout, float* packed, void* stream);

/* out[b, y, x, co] = act( conv7x7_s2_p3(in)[b, co, y, x] * scale[co] + shift[co] ): encoder.conv1 + bn1 (eval mode:
 * scale = weight / sqrt(running_var + eps), shift = bias - running_mean * scale; NULL = identity) + ReLU
 * (leaky_slope = 0; < 0: no activation) -- reference networks.py:176-179.  `in` is the image with arbitrary element
 * strides (NCHW or channels-last), `out` is channels-last [B, H/2, W/2, 64]. */
int sr_stem7x7_fwd(const float* in, int64_t in_batch_stride, int64_t in_chan_stride, int64_t in_row_stride,
                   int64_t in_col_stride, const float* packed_weight, const float* scale, const float* shift,
                   float leaky_slope, float* out, int64_t out_batch_stride, int out_pix_stride, int B, int H, int W,
                   int Cout, void* stream);

/* encoder.maxpool of the antialiased backbone: nn.MaxPool2d(kernel_size=2, stride=1) followed by
 * BlurPool(filt_size=4, stride=2, reflect padding (1,2,1,2), taps outer([1,3,3,1])/64), fused.
 * [B,H,W,C] -> [B,(H-2)/2+1,(W-2)/2+1,C] channels-last, C % 4 == 0, H, W >= 4. */
int sr_maxblurpool_nhwc_fwd(const float* in, int64_t in_batch_stride, int in_pix_stride, float* out,
                            int64_t out_batch_stride, int out_pix_stride, int B, int H, int W, int C, void* stream);

/* nn.InstanceNorm2d(C) (affine=False, biased variance over H*W per image and channel) optionally followed by
 * LeakyReLU(leaky_slope) (< 0: none) -- reference networks.py:188-189, 198.  Deterministic (no atomics); `out` may
 * alias `in`.  C % 4 == 0, C <= 256.  Workspace: sr_instance_norm_workspace_bytes, 16-byte aligned. */
size_t sr_instance_norm_workspace_bytes(int B, int H, int W, int C);
int sr_instance_norm_nhwc_fwd(const float* in, int64_t in_batch_stride, int in_pix_stride, float* out,
                              int64_t out_batch_stride, int out_pix_stride, int B, int H, int W, int C, float eps,
                              float leaky_slope, void* workspace, size_t workspace_bytes, void* stream);

/* Statistics only: stats[b][0][c] = mean, stats[b][1][c] = 1 / sqrt(var + eps) ([B,2,C] floats, 16-byte aligned) -- for
 * consumers that normalise on the fly (sr_conv3x3_c16_nhwc_fwd).  Same workspace as sr_instance_norm_nhwc_fwd. */
int sr_instance_norm_stats_nhwc(const float* in, int64_t in_batch_stride, int in_pix_stride, int B, int H, int W, int C,
                                float eps, float* stats, void* workspace, size_t workspace_bytes, void* stream);

/* Conv2d(64, 128, 1) + bias AND the InstanceNorm2d statistics of its output in one pass (reference
 * modules/networks.py:187-188): `out` is the raw convolution, `stats` [B,2,128] = (mean, 1 / sqrt(var + eps)) as
 * sr_instance_norm_stats_nhwc would compute them from `out`.  weight [128][64] (the module's own layout, no packing).
 * Other channel counts: SR_ERR_UNSUPPORTED (callers run sr_conv1x1 + sr_instance_norm_stats_nhwc instead). */
size_t sr_conv1x1_stats_workspace_bytes(int B, int H, int W, int Cout);
int sr_conv1x1_stats_nhwc_fwd(const float* in, int64_t in_batch_stride, int in_pix_stride, const float* weight,
                              const float* bias, float* out, int64_t out_batch_stride, int out_pix_stride, int B, int H,
                              int W, int Cin, int Cout, float eps, float* stats, void* workspace, size_t workspace_bytes,
                              void* stream);

/* nn.Conv2d(Cin, Cout <= 16, 3, padding=1, padding_mode = replicate ? "replicate" : "zeros") + bias [+ LeakyReLU] on
 * channels-last data, with an optional InstanceNorm (+ LeakyReLU(in_leaky_slope)) applied to the INPUT on the fly from
 * `in_stats` (sr_instance_norm_stats_nhwc; NULL = input used as is): the InstanceNorm -> LeakyReLU -> Conv2d(128, 16,
 * replicate) end of the matching encoder (reference modules/networks.py:188-197) without materialising the
 * normalised tensor.  Cin % 32 == 0; fp32 MFMA 16x16x4 (no padded output channels). */
size_t sr_conv3x3_c16_packed_weight_floats(int Cout, int Cin);
int sr_conv3x3_c16_pack_weights(const float* weight, int Cout, int Cin, float* packed, void* stream);
int sr_conv3x3_c16_nhwc_fwd(const float* in, int64_t in_batch_stride, int in_pix_stride, const float* in_stats,
                            float in_leaky_slope, const float* packed_weight, const float* bias, float* out,
                            int64_t out_batch_stride, int out_pix_stride, int B, int H, int W, int Cin, int Cout,
                            int replicate, float leaky_slope, void* stream);

/* ------------------------------------------------------------- TSDF fusion -----------
 *
 * TSDFFuser.integrate_depth (reference tools/tsdf.py:238-320; project_to_camera :218-236; voxel coordinates of
 * TSDF.from_bounds / generate_voxel_coords :69-111): fuses a batch of B depth maps, in order, into the fp16 TSDF volume.
 * All tensors are fp16 as the reference feeds them (OurFuser.fuse_frames, tools/fusers_helper.py:62-68); results are
 * bit-identical to the reference executed on CPU.
 *
 *  tsdf_values, tsdf_weights : [X,Y,Z] fp16, contiguous (z fastest), updated in place; Z % 8 == 0 (the reference rounds
 *                              volume dimensions to multiples of 8, tsdf.py:16,80-85), 16-byte aligned
 *  voxel_coords              : [3,X,Y,Z] fp16 explicit world coordinates, or NULL: origin + index * voxel_size
 *                              (fp32, rounded to fp16) as TSDF.from_bounds generates them -- saves 6 of 10 bytes/voxel
 *  depth [B,H,W] fp16, depth_mask [B,H,W] bool or NULL, K / T [B,4,4] fp16 row-major (intrinsics, cam_T_world)
 *  min_depth, max_depth, truncation (= truncation_size * voxel_size), maxW: the fuser's python scalars as fp32;
 *  depth_range = max_depth - min_depth evaluated in double, as fp32.
 *  B <= 1024 per call (per-frame state in LDS: 48 B + 16 ceil(B / 16) bytes), else SR_ERR_UNSUPPORTED; the update is
 *  sequential per voxel, so a longer batch is exactly consecutive calls over consecutive frames (TSDFFuser.integrate_depth
 *  splits it that way).
 */
int sr_tsdf_integrate_fwd(void* tsdf_values, void* tsdf_weights, const void* voxel_coords, int X, int Y, int Z,
                          float origin_x, float origin_y, float origin_z, float voxel_size, const void* depth,
                          const uint8_t* depth_mask, const void* K, const void* T, int B, int H, int W,
                          float min_depth, float max_depth, float depth_range, float truncation, float maxW,
                          void* stream);

/* ------------------------------------------------------------- mesh extraction -------
 *
 * Marching cubes on a fused TSDF volume (the reference's TSDF.to_mesh, tools/tsdf.py:128-156, runs skimage on the host
 * with level = 0, values clamped to [-1, 1] and allow_degenerate = False).  Output: an indexed mesh with shared vertices.
 *
 *  tsdf_values : [X,Y,Z] fp16, contiguous (z fastest), X, Y, Z >= 2.  Z % 8 == 0 with 16-byte alignment takes 16-byte
 *                loads; other shapes a scalar path with the same results.
 *
 * Rules (tests/mesh_oracle.py implements them in numpy):
 *  - Corners: fp16 -> fp32, clamped to [-1, 1]; a corner is below if v < level, else above.  An edge with a NaN endpoint
 *    has no vertex; a cube with a NaN corner emits nothing.
 *  - Vertices: voxel (i,j,k) owns its edges toward +x, +y, +z.  An edge with endpoints on different sides has one vertex
 *    at p0 + t along its axis, t = (level - v0) / (v1 - v0), v0 the lower-index endpoint.  Vertices are numbered in
 *    linear voxel order, then x, y, z edge order (independent of the schedule).
 *  - Faces of a cube: 2 or 4 crossing edges.  With 4 (above corners a, c on one diagonal, below b, d on the other, all
 *    minus level) the above corners are joined across the face iff a*c >= b*d (fp32, no FMA): the asymptotic decider.
 *    It depends on the face's own values only, so neighbouring cubes agree and the mesh has no cracks.
 *  - Loops: the face segments chain into closed loops, oriented so that triangles wind counter-clockwise seen from the
 *    above side (face normals point toward increasing TSDF).  Each loop is a fan from its vertex with the smallest global
 *    index; a triangle is dropped if two of its three voxel-unit positions are bitwise equal.
 *  - Coordinates: origin + p * scale in fp32 (scale_to_world: the fp16 origin as fp32 and the voxel size; else 0 and 1).
 *    normals (optional): central-difference gradients of the clamped values at both endpoints (one-sided at the border),
 *    g0 + t * (g1 - g0), normalised; a zero gradient gives a zero normal.
 *
 * Use: sr_mesh_count writes {active voxels, vertices, triangles} as int64 to the device array `totals`[3] and brick
 * offsets to `count_scratch` (sr_mesh_count_scratch_bytes, 16-byte aligned).  After the host has read the totals,
 * sr_mesh_emit with the same volume, level and count_scratch, a `list_scratch` of sr_mesh_list_scratch_bytes(active)
 * bytes (16-byte aligned) writes vertices [V,3] fp32, normals [V,3] fp32 (NULL: none) and faces [F,3] int32.
 * V or F >= 2^31: SR_ERR_UNSUPPORTED.  The library allocates nothing; no host synchronisation inside either call. */
size_t sr_mesh_count_scratch_bytes(int X, int Y, int Z);
size_t sr_mesh_list_scratch_bytes(int64_t active);
int sr_mesh_count(const void* tsdf_values, int X, int Y, int Z, float level, void* count_scratch,
                  size_t count_scratch_bytes, int64_t* totals, void* stream);
int sr_mesh_emit(const void* tsdf_values, int X, int Y, int Z, float level, float origin_x, float origin_y, float origin_z,
                 float scale, const void* count_scratch, size_t count_scratch_bytes, void* list_scratch,
                 size_t list_scratch_bytes, int64_t active, int64_t num_vertices, int64_t num_faces, float* vertices,
                 float* normals, int* faces, void* stream);

/* ------------------------------------------------------------- point-cloud fusion ----
 *
 * Multi-view consistency fusion of predicted depth maps into a point cloud (the reference's pc_fusion.py with
 * tools/torch_point_cloud_fusion.py:12-118, a Python loop over [100, 3, h*w] torch temporaries), then open3d's voxel
 * downsampling.  tests/pc_oracle.py implements the same rules in fp64 numpy.
 *
 * Inputs of a scene of N frames: depth D [N,h,w] fp32; intrinsics K [N,3,3]; world-to-camera poses P [N,4,4]
 * (cam_T_world), P_i = [R_i | t_i].
 *
 * Rules, per reference frame r.  Its sources are every other frame s != r, in ascending index.  For each pixel
 * (u = column, v = row, integers) with depth d = D_r[v,u]:
 *  1. World point X = P_r^-1 (K_r^-1 (u*d, v*d, d)) as a 3-D point, for every d: a zero depth is not excluded and
 *     gives the camera centre.
 *  2. Projection into s: q = K_s (R_s X + t_s), z = q_z, x = q_x / z, y = q_y / z.
 *  3. In bounds: z > 1e-4, 0 <= x <= w-1, 0 <= y <= h-1 (continuous coordinates, closed intervals).
 *  4. Sampled depth z_s: the nearest texel of D_s as grid_sample(mode="nearest", align_corners=True, zeros padding)
 *     picks it: (x, y) normalised to [-1, 1] and back, ((g + 1) / 2) * (size - 1), rounded half to even.  A zero in
 *     D_s is an ordinary value (a source sampled at 0 is consistent when z < z_thresh).
 *  5. Source s is consistent when it is in bounds and |z - z_s| < z_thresh (strict).  n = number of consistent sources.
 *  6. Sampled point Y_s = R_s^T (K_s^-1 (x*z_s, y*z_s, z_s) - t_s), at the continuous (x, y), not the texel centre.
 *  7. avg = (X + sum of Y_s) / (n + 1): the sum runs over the consistent sources whose Y_s has no NaN component, in
 *     the order X, then s ascending.  The reference frame's own point is always in it.
 *  8. The pixel is kept when n >= n_consistent_thresh.  Kept points are listed frame by frame, each frame row-major;
 *     a point's colour is the reference frame's uint8 image at [v,u]; the keep masks [N,h,w] are an output too.
 *
 * Voxel downsampling (open3d's voxel_down_sample, restated): in fp64, min_bound = the per-axis minimum of the points
 * - voxel_size / 2; voxel index = floor((p - min_bound) / voxel_size) with IEEE fp64 division.  Each occupied voxel
 * gives one point, the fp64 mean of its points cast to fp32, and one colour, the integer mean of its uint8 colours
 * rounded half up: (sum + cnt / 2) / cnt (our definition; open3d keeps float colours).  Voxels come out in ascending
 * key = ix * 2^42 + iy * 2^21 + iz; an extent of 2^21 voxels or more on an axis is refused by the caller.
 *
 * sr_pc_consistency: one launch fuses the reference frames [ref_begin, ref_begin + ref_count) against all N frames.
 *  depth        [N,h,w] fp32
 *  frame_consts [N, SR_PC_FRAME_FLOATS] fp32, computed by the caller in fp64, per frame i:
 *               [0,12)  K_i [R_i | t_i]                 (3x4 row-major: step 2 as one affine map)
 *               [12,21) R_i^T K_i^-1, [21,24) -R_i^T t_i (step 6: Y = z_s * (R^T K^-1 (x, y, 1)) - R^T t)
 *               [24,33) P_i^-1[:3,:3] K_i^-1, [33,36) P_i^-1[:3,3]  (step 1, for i as the reference frame)
 *  points       [ref_count,h,w,3] fp32: avg of step 7 for every pixel (kept or not)
 *  counts       [ref_count,h,w] int32: n of step 5
 * The rules are evaluated in fp32 with these fused constants, and the texel is the nearest one to the continuous
 * (x, y) (the normalisation round trip of step 4 moves a coordinate by a few ulps only), so decisions within rounding
 * distance of a threshold or of a texel boundary may differ from the reference's fp32 evaluation.  No atomics: each
 * pixel's sum is kept in registers in source order, so results do not depend on the schedule.
 * Refused (SR_ERR_INVALID_ARGUMENT): a NULL pointer, N < 1, h or w < 2, an empty or out-of-range chunk, h*w*3*4 bytes
 * or ref_count*h*w*3*4 bytes beyond int32 indexing, z_thresh not positive and finite.
 *
 * sr_pc_voxel_keys: keys [M] int64 of points [M,3] fp32 for the given fp64 min_bound and voxel_size (indices clamped
 * to [0, 2^21)).  sr_pc_voxel_mean: given the stable key-sorted permutation `order` [M] int64 and the run starts
 * `seg_start` [S+1] int64 (seg_start[S] = M), writes out_points [S,3] fp32 and, when colors [M,3] uint8 is not NULL,
 * out_colors [S,3] uint8: a thread per voxel sums its points in sorted order.  None of the three calls takes scratch;
 * the library allocates nothing and does not synchronise the host. */
#define SR_PC_FRAME_FLOATS 36
int sr_pc_consistency(const float* depth, const float* frame_consts, int N, int h, int w, int ref_begin, int ref_count,
                      float z_thresh, float* points, int* counts, void* stream);
int sr_pc_voxel_keys(const float* points, int64_t M, double min_x, double min_y, double min_z, double voxel_size,
                     int64_t* keys, void* stream);
int sr_pc_voxel_mean(const float* points, const uint8_t* colors, int64_t M, const int64_t* order,
                     const int64_t* seg_start, int64_t S, float* out_points, uint8_t* out_colors, void* stream);

/* ------------------------------------------------------------- training losses ----
 *
 * The reference's training objective (experiment_modules/depth_model.py:409-500 `compute_losses`, losses.py and
 * utils/geometry_utils.py:92-133 `NormalGenerator`), forward and backward.  Everything is fp32 in and fp32 out, and
 * gradients flow to the predictions only: gt depth, masks, poses and intrinsics are data.  tests/loss_oracle.py
 * restates the rules in fp64 torch.  Maps are dense [B,h,w] (a [B,1,h,w] tensor), normals [B,3,h,w], matrices
 * row-major [.,4,4].  Refused (SR_ERR_INVALID_ARGUMENT): a NULL pointer, B < 1 or B > 65535, h or w < 3 (the
 * 5x5 reflect blur needs 3), h*w > 2^28, K outside [1, SR_LOSS_MAX_SOURCES]; a scratch smaller than its query:
 * SR_ERR_WORKSPACE_TOO_SMALL.  Scratch sizes come from the *_workspace_bytes queries (0 for a refused shape); the
 * library allocates nothing.
 *
 * Three kornia 0.6.7 filters are restated (the reference pins that version):
 *  - blur_pool2d(x, 3): correlation with [1,2,1]^T [1,2,1] / 16, zero padding 1, stride 2: n pixels -> ceil(n/2).
 *    The gradient loss's pyramid has 4 levels; level 0 is the map itself.
 *  - spatial_gradient(x): Sobel / 8 with replicate borders.  gx = correlation with [[-1,0,1],[-2,0,2],[-1,0,1]] / 8
 *    (positive when values grow with x), gy with its transpose.  A component is non-finite when any of its nine
 *    taps is, zero-weight taps included (ATen's conv: NaN * 0 = NaN).
 *  - gaussian_blur2d(x, (5,5), (2,2)): weights exp(-t^2/8), t in -2..2, normalised to sum 1, applied as their 5x5
 *    outer product, `reflect` padding of 2 (no edge repeat).
 *
 * Rules:
 *  - Normals (NormalGenerator): blur the depth, back-project it (pixel centres at +0.5: P = s * invK[:3,:3] (x+.5,
 *    y+.5, 1)), take spatial_gradient of the 3 point channels; n = c / max(|c|, 1e-12), c = cross(gx, gy).
 *  - NormalsLoss: mask = all three components finite in gt and in pred; loss = masked mean of 0.5 (1 - n_pred . n_gt).
 *  - MSGradientLoss: the sum over the 4 pyramid levels of the mean |grad pred - grad gt| over the gradient components
 *    (x and y separately) whose gt value is finite.  On depth, not log depth.  An empty level gives NaN.
 *  - MVDepthLoss, per source k: back-project gt, move it to world (cur_world_T_cam), project into k (K_k cam_T_world_k,
 *    z' = q_z + eps, pixel = q_xy / z' when |q_z| > eps, else q_xy); sample the source gt depth nearest as
 *    grid_sample(align_corners=False, zeros) does: normalise to [-1, 1] and back, round half to even, 0 out of bounds.
 *    Valid: z' < 1.05 s, z' > 0, s > 0 (NaN fails all three).  Error |log s - log z'_pred| with z'_pred the predicted
 *    depth through the same chain.  mean over the valid pixels whose error is not NaN (nanmean) per k, then the mean
 *    over k.  An empty k gives NaN, exactly as the reference; its gradient contribution is zero.
 *  - Depth terms, all on mask_b: ms = sum_i mean |log gt - NN_i(log_pred_s{i})| / 2^i over the scales present (NN_i:
 *    F.interpolate(mode="nearest") to gt size, source index min(floor(dst * (in/out)), in - 1) in fp32); abs, log_l1,
 *    si = sqrt(mean d^2 - lambda (mean d)^2) with d = log gt - log_pred_s0; inv_abs on mask_b & depth_pred > 0.1.
 * The gradient of |x| at 0 is 0.
 *
 * Execution: every loss writes fixed-order per-block partials to the scratch and one single-workgroup finalize sums
 * them in fp64 into `out` on the device: no float atomics (two runs give the same bits) and no host synchronisation;
 * the backward entry points read the incoming gradient(s) and the forward's `out` (counts, means) from device
 * memory.  The launch count does not depend on K.
 *
 * sr_normals_fwd / _bwd: depth [B,h,w], invK [B,4,4] -> normals [B,3,h,w]; grad_normals -> grad_depth [B,h,w].
 * sr_normals_loss_fwd: out[2] = {loss, count}.  _bwd: grad_pred [B,3,h,w] of the scalar grad_out[0].
 * sr_grad_loss_fwd: out[5] = {loss, count of levels 0..3}.  _bwd reads the pyramid the forward left in the scratch:
 *   pass the same scratch, unchanged.
 * sr_mv_loss_fwd: src_depth [B,K,h,w], src_K / src_cam_T_world [B,K,4,4]; out[1 + 2K] = {loss, count_k, mean_k};
 *   valid_mask [B,K,h,w] uint8 and sampled [B,K,h,w] (the sampled source depth) are optional (NULL: not written).
 * sr_depth_terms_fwd: mask_b [B,h,w] uint8 (0 / 1), log0 [B,h,w] is required, log1..3 [B,h_i,w_i] may be NULL
 *   (h_i <= h, w_i <= w); out[8] = {ms, abs, inv_abs, log_l1, si, count, inv count, mean d}.  _bwd: grad_outs[5] =
 *   d{ms, abs, inv_abs, log_l1, si}; writes grad_depth_pred and the grad of every present log scale.  gt_is_log != 0:
 *   depth_gt holds log depth already (ScaleInvariantLoss on its own; abs and inv_abs are then meaningless).  These
 *   two take any h, w >= 1. */
#define SR_LOSS_MAX_SOURCES 15
size_t sr_normals_workspace_bytes(int B, int h, int w);
int sr_normals_fwd(const float* depth, const float* invK, int B, int h, int w, float* normals, void* scratch,
                   size_t scratch_bytes, void* stream);
int sr_normals_bwd(const float* grad_normals, const float* depth, const float* invK, int B, int h, int w,
                   float* grad_depth, void* scratch, size_t scratch_bytes, void* stream);
size_t sr_normals_loss_workspace_bytes(int B, int h, int w);
int sr_normals_loss_fwd(const float* normals_gt, const float* normals_pred, int B, int h, int w, float* out,
                        void* scratch, size_t scratch_bytes, void* stream);
int sr_normals_loss_bwd(const float* grad_out, const float* stats, const float* normals_gt, const float* normals_pred,
                        int B, int h, int w, float* grad_pred, void* stream);
size_t sr_grad_loss_workspace_bytes(int B, int h, int w);
int sr_grad_loss_fwd(const float* depth_gt, const float* depth_pred, int B, int h, int w, float* out, void* scratch,
                     size_t scratch_bytes, void* stream);
int sr_grad_loss_bwd(const float* grad_out, const float* stats, const float* depth_gt, const float* depth_pred, int B,
                     int h, int w, float* grad_pred, void* scratch, size_t scratch_bytes, void* stream);
size_t sr_mv_loss_workspace_bytes(int B, int K, int h, int w);
int sr_mv_loss_fwd(const float* depth_pred, const float* depth_gt, const float* src_depth, const float* cur_invK,
                   const float* src_K, const float* cur_world_T_cam, const float* src_cam_T_world, int B, int K, int h,
                   int w, float eps, float* out, uint8_t* valid_mask, float* sampled, void* scratch,
                   size_t scratch_bytes, void* stream);
int sr_mv_loss_bwd(const float* grad_out, const float* stats, const float* depth_pred, const float* depth_gt,
                   const float* src_depth, const float* cur_invK, const float* src_K, const float* cur_world_T_cam,
                   const float* src_cam_T_world, int B, int K, int h, int w, float eps, float* grad_pred,
                   void* stream);
size_t sr_depth_terms_workspace_bytes(int B, int h, int w);
int sr_depth_terms_fwd(const float* depth_gt, const uint8_t* mask_b, const float* depth_pred, const float* log0,
                       const float* log1, int h1, int w1, const float* log2, int h2, int w2, const float* log3, int h3,
                       int w3, int B, int h, int w, float si_lambda, int gt_is_log, float* out, void* scratch,
                       size_t scratch_bytes, void* stream);
int sr_depth_terms_bwd(const float* grad_outs, const float* stats, const float* depth_gt, const uint8_t* mask_b,
                       const float* depth_pred, const float* log0, const float* log1, int h1, int w1,
                       const float* log2, int h2, int w2, const float* log3, int h3, int w3, int B, int h, int w,
                       float si_lambda, int gt_is_log, float* grad_depth_pred, float* grad_log0, float* grad_log1, float* grad_log2,
                       float* grad_log3, void* stream);

/* ------------------------------------------------------------- depth metrics ------
 *
 * The reference's depth metrics (utils/metrics_utils.py `compute_depth_metrics_batched`, used per test batch by
 * test.py:203-455, and `compute_depth_metrics`, used by the validation step, experiment_modules/depth_model.py:573-596).
 * tests/metrics_oracle.py restates the rules in numpy.
 *
 *  gt    [B,H,W]  ground-truth depth;  pred [B,h,w] predicted depth;  mask [B,H,W] uint8 (0 / nonzero) or NULL.
 *  valid: mask != 0 when a mask is given, else gt > min_depth (fp32 compare; a NaN gt is not valid; test.py uses 0.5).
 *  resample: SR_RESAMPLE_IDENTITY (h == H and w == W) or SR_RESAMPLE_NEAREST: gt pixel (y, x) reads pred at the pixel
 *    F.interpolate(mode="nearest") picks, per axis src = dst if in == out, dst >> 1 if out == 2 in, else
 *    min((int)floorf((float)dst * ((float)in / (float)out)), in - 1).  The resampled map is never written.
 *
 * Per valid pixel, fp32 in the reference's operation order: d = gt - pred; the five error terms |d|, |d| / gt,
 * d * d / gt, d * d, (logf(gt) - logf(pred))^2; ratio = max(gt / pred, pred / gt), NaN when either quotient is NaN
 * (torch.max).  Sums and counts are fp64.
 * Rules:
 *  - Batched rule (per frame, out_frame): invalid pixels are dropped from everything.  Each error metric is the mean of
 *    its term over the valid pixels where that term is not NaN (nanmean), so each metric has its own count; a metric
 *    with no such pixel (a frame with no valid pixel included) is NaN.  rmse = sqrt(mean d^2), rmse_log =
 *    sqrt(mean log^2), the square root taken in fp64 on the fp64 mean before rounding to fp32.
 *  - Accuracy: a_t = (number of valid pixels with ratio < t) / (number of valid pixels), rounded to fp32; a NaN ratio
 *    is not accurate.  The thresholds compare in fp32: 1.05f (a5), 1.1f (a10, and a0 = a10), 1.25f (a25, and
 *    a1 = a25), 1.5625f (a2), 1.953125f (a3); a ratio exactly (float)1.05 is not in a5.  mult_a != 0 multiplies them
 *    by 100.0f in fp32 after the division.
 *  - Quirks kept: pred < 0 (gt > 0) makes both quotients negative, so the pixel is accurate in every a-metric, while
 *    logf(pred) is NaN and the pixel leaves rmse_log only.  pred == 0: ratio = inf (not accurate), log term inf.  pred
 *    NaN: the pixel leaves the five error means and is not accurate.  pred = inf: the error metrics are inf.
 *  - Pooled rule (out_pooled, `compute_depth_metrics` on the selection of every valid pixel of the batch): the same
 *    terms with plain means: a NaN term makes its metric NaN; no valid pixel makes every metric NaN.
 *  - Outputs: out_frame [B,12] in the reference's key order abs_diff, abs_rel, sq_rel, rmse, rmse_log, a5, a10, a25,
 *    a0, a1, a2, a3; out_count [B] int32, the valid pixels of each frame; out_pooled [12] in the same order, or NULL.
 *
 * Execution: a block per (frame, tile of 4096 gt pixels) writes one fixed-order fp64 record to the scratch, and one
 * single-workgroup finalize reduces a frame's records in a fixed order and the frames' totals in frame order: no float
 * atomics, no host synchronisation, two runs give the same bits, and since a frame's records depend only on (H, W, h,
 * w), frame b gives the same bits scored alone or in any batch.  Two launches per call.
 * Refused (SR_ERR_INVALID_ARGUMENT): a NULL gt, pred, out_frame, out_count or scratch; B < 1 or B > 65535; an empty
 * map; H*W or h*w above SR_METRICS_MAX_PIXELS (2^24: counts stay exact in fp32 and int32); identity with h != H or
 * w != W; an unknown resample mode.  A scratch smaller than sr_depth_metrics_workspace_bytes(B, H, W) (0 for a refused
 * shape): SR_ERR_WORKSPACE_TOO_SMALL.  The library allocates nothing.
 *
 * sr_depth_metrics_gather (tests only): writes out [B,H,W] = pred read through the index map of `resample`, the same
 * device code the metrics use. */
#define SR_RESAMPLE_IDENTITY 0
#define SR_RESAMPLE_NEAREST 1
#define SR_METRICS_MAX_PIXELS (1 << 24)
size_t sr_depth_metrics_workspace_bytes(int B, int H, int W);
int sr_depth_metrics(const float* gt, const float* pred, const uint8_t* mask, float min_depth, int B, int H, int W,
                     int h, int w, int resample, int mult_a, float* out_frame, int32_t* out_count, float* out_pooled,
                     void* scratch, size_t scratch_bytes, void* stream);
int sr_depth_metrics_gather(const float* pred, int B, int H, int W, int h, int w, int resample, float* out,
                            void* stream);

/* ------------------------------------------------------------- mesh metrics -------
 *
 * Scores a reconstruction against a ground truth as TransformerFusion's / NeuralRecon's mesh evaluation does (the
 * reference README's "Mesh Fusion" table): exact nearest neighbours between two point sets, area-weighted sampling of a
 * triangle mesh, and the Acc / Comp / Chamfer / Precision / Recall / F-score reduction.  tests/mesh_metrics_oracle.py
 * restates every rule in numpy.  Point sets are dense [n,3] fp32; counts are below 2^31.
 *
 * Nearest neighbour.  For every query q of Q [M,3] and the targets P [N,3] (N >= 1):
 *  - d2 = (dx*dx + dy*dy) + dz*dz in fp32 with dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z, each operation rounded
 *    on its own (no FMA contraction).  out_d2 = the minimum of d2 over all N targets, bit for bit; out_index = the
 *    smallest target index among the targets with that d2 (numpy's argmin); out_dist = sqrtf(out_d2), correctly
 *    rounded (numpy's fp32 np.sqrt).  The library's sqrtf is the correctly rounded one at -O3 -fno-fast-math; the
 *    __fsqrt_rn intrinsic of this toolchain is the bare hardware approximation and is not used.
 *  - Grid (sr_nn_grid_plan, on the host): the targets' box [min, max] (fp64, from the caller), extents e_a, E = max
 *    e_a.  Fine cell edge h: E * 0.8^k for the smallest k in [0, 200) with prod_a (floor(e_a / h) + 1) >= N (about one
 *    target per cell), then h * 1.25^j for the smallest j in [0, 200) whose table fits max_cells; E = 0 gives h = 1.
 *    dims g_a = floor(e_a / h) + 1.  A coarse cell is 8^3 fine cells; the table holds 512 * prod_a ceil(g_a / 8)
 *    <= max_cells <= SR_NN_MAX_CELLS (2^26) cells, plus one entry.
 *  - Cell of a point: t_a = (p_a - min_a) / h in fp64, c_a = floor(t_a) clamped into [0, g_a).  Key = (coarse cell,
 *    row-major over (x, y, z) coarse indices) * 512 + (c_x & 7) * 64 + (c_y & 7) * 8 + (c_z & 7).
 *  - Search: Chebyshev shells of fine cells around the query's cell, r < SR_NN_FINE_SHELLS, then shells of coarse
 *    cells until the whole grid is covered.  After every shell the query stops when its best d2 is strictly below a
 *    lower bound of the fp32 d2 of every target outside the searched box, and a coarse cell is skipped when its own
 *    lower bound is strictly above the best d2; both bounds hold after rounding (relative margin 2^-18; the argument is
 *    in csrc/sr_meshmetrics.hip).  Loops are bounded by the grid dimensions and N.
 *  - Coordinates must be finite with |x| <= SR_NN_MAX_COORD (1e18: d2 cannot overflow).  The caller passes the boxes
 *    of both sets; a non-finite box, or one beyond the limit, is SR_ERR_INVALID_ARGUMENT.
 * Use: sr_nn_grid_plan -> sr_nn_keys(targets) -> a stable sort of the keys (the caller's: torch.sort) ->
 * sr_nn_build (sorted targets [N,4] fp32 = (x, y, z, bits of the int32 index), 16-byte aligned, and the cell-start
 * table [table_entries] int32) -> sr_nn_query.  Queries may be visited in any order (query_order [M] int64, a
 * permutation, or NULL); sorting them by sr_nn_keys keeps the lanes of a wave in neighbouring cells.  Results do not
 * depend on the order.  out_d2, out_dist and out_index [M] are each optional.
 *
 * Surface sampling.  sr_sample_surface_cdf writes cdf [F] fp64, the inclusive prefix sum of the face areas
 * 0.5 |(B - A) x (C - A)| (fp64 from the fp32 vertices), summed in a fixed order: chunks of 64 faces in face order, the
 * chunk totals in chunk order in 256 contiguous slices.  Faces with an index outside [0, V) count as zero area (the
 * caller refuses them).  sr_sample_surface then writes n points, sample i:
 *    s = mix(seed), h_k = mix(s ^ (3 i + k)) for k = 0, 1, 2, in uint64 with wrap-around, where mix is splitmix64's
 *    finaliser: z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) *
 *    0x94D049BB133111EB; z ^ (z >> 31).
 *    x = (double)(h_0 >> 12) * 2^-52 * total (fp64, < total); face = the smallest f with cdf[f] > x, so a zero-area
 *    face is never chosen.  u = (h_1 >> 40) * 2^-24, v = (h_2 >> 40) * 2^-24 (fp32, in [0, 1)); s = sqrtf(u);
 *    a = 1 - s, b = s * (1 - v), c = s * v; p = (a * A + b * B) + c * C per coordinate in fp32.
 * out_face [n] int32 (optional) receives the face.  A zero total area is refused by the caller.
 *
 * Metrics.  dist_pred_to_gt [m] and dist_gt_to_pred [n] are nearest-neighbour distances; threshold t > 0.  Per block
 * of 4096 distances, fixed-order fp64 sums of the distances and of the count with dist < t (strict, fp32 compare),
 * then one single-workgroup finalize writes out[8] fp64 = {acc = mean pred->gt, comp = mean gt->pred, chamfer =
 * (acc + comp) / 2, precision = fraction of pred within t, recall = fraction of gt within t, f_score = 2PR / (P + R)
 * (0 when P + R is 0), count of pred within t, count of gt within t}.  m = 0 (an empty prediction; dist_gt_to_pred is
 * then not read): acc and precision NaN, comp and chamfer +inf, recall 0, f_score 0.  n must be >= 1.
 *
 * No float atomics (two runs give the same bits) and no host synchronisation in any call; the library allocates
 * nothing.  Refused (SR_ERR_INVALID_ARGUMENT): NULL required pointers, counts outside their range, a grid whose table
 * exceeds SR_NN_MAX_CELLS or does not have table_entries entries, a misaligned buffer; a scratch smaller than its query: SR_ERR_WORKSPACE_TOO_SMALL. */
#define SR_NN_MAX_CELLS (1 << 26)
#define SR_NN_FINE_SHELLS 3
#define SR_NN_MAX_COORD 1e18
int sr_nn_grid_plan(int64_t n_targets, const double* target_box /* host [6]: min x, y, z, max x, y, z */,
                    int64_t max_cells, double* cell /* host */, int* dims /* host [3] */,
                    int64_t* table_entries /* host */);
int sr_nn_keys(const float* points, int64_t n, double min_x, double min_y, double min_z, double cell, int gx, int gy,
               int gz, int32_t* keys, void* stream);
int sr_nn_build(const float* targets, int64_t n, const int32_t* sorted_keys, const int64_t* order,
                int64_t table_entries, float* sorted_targets, int32_t* cell_start, void* stream);
int sr_nn_query(const float* queries, int64_t m, const int64_t* query_order, const float* sorted_targets, int64_t n,
                const int32_t* cell_start, int64_t table_entries, double min_x, double min_y, double min_z, double cell,
                int gx, int gy, int gz, float* out_d2, float* out_dist, int32_t* out_index, void* stream);
size_t sr_sample_surface_workspace_bytes(int64_t num_faces);
int sr_sample_surface_cdf(const float* vertices, int64_t num_vertices, const int32_t* faces, int64_t num_faces,
                          double* cdf, void* scratch, size_t scratch_bytes, void* stream);
int sr_sample_surface(const float* vertices, int64_t num_vertices, const int32_t* faces, int64_t num_faces,
                      const double* cdf, int64_t n, uint64_t seed, float* out_points, int32_t* out_face, void* stream);
size_t sr_mesh_metrics_workspace_bytes(int64_t m, int64_t n);
int sr_mesh_metrics(const float* dist_pred_to_gt, int64_t m, const float* dist_gt_to_pred, int64_t n, float threshold,
                    double* out, void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------- sparse TSDF --------
 *
 * Sparse colour TSDF fusion: the reference's second depth fuser (tools/fusers_helper.py, Open3DFuser, on Open3D's legacy
 * ScalableTSDFVolume with RGB8 colour).  The volume is a set of blocks of 16^3 voxels that grows where the depth maps
 * land.  The rules below restate Open3D's integrate / extract_triangle_mesh from memory of its algorithm: they are this
 * project's contract, and bit parity with Open3D itself is unpinned (nobody could check it against Open3D).
 * tests/sparse_tsdf_oracle.py restates every rule in numpy.
 *
 * Parameters: voxel_length vl, sdf_trunc (3 vl for the fuser), unit = 16 vl; 2 sdf_trunc < unit.
 * Block key: (bx, by, bz) with each coordinate in [-2^20, 2^20), key = (bx + 2^20) << 42 | (by + 2^20) << 21 |
 * (bz + 2^20) >= 0: ascending keys are x-major order.  SR_STSDF_KEY_NONE (-1) marks an empty candidate.
 * Voxel l of a block (l = (lx * 16 + ly) * 16 + lz, z fastest) has the global index g = 16 b + (lx, ly, lz).
 * Pool: [capacity][5][4096] fp32 per block slot: tsdf, weight, red, green, blue (0..255).  Fresh blocks are all zero.
 * A frame's depth D [h,w] fp32 has already had values above max_depth set to 0 (the caller's preprocessing).
 *
 * Touch (fp64; sr_stsdf_touch).  Pixels (u, v) with u % 4 == 0, v % 4 == 0 and d > 0 (NaN fails): p_cam = ((u - cx) d
 * / fx, (v - cy) d / fy, d); p_world = M p_cam with M = inv(cam_T_world) rows 0..2, computed by the caller in fp64,
 * each row ((m0 x + m1 y) + m2 z) + m3.  Per axis lo = floor((p - sdf_trunc) / unit), hi = floor((p + sdf_trunc) /
 * unit); every block in [lo, hi]^3 is touched by the frame.  A non-finite p_world or a block outside the key range is
 * skipped.  Output cand_keys [B][S][8] int64, S = ceil(h/4) * ceil(w/4), pixel-major: the up to 8 blocks of the
 * pixel, SR_STSDF_KEY_NONE for the rest.
 * Touch masks (sr_stsdf_block_masks): masks[inverse[i]] |= 1 << (i / cand_per_frame) for every candidate i that is
 * not SR_STSDF_KEY_NONE (inverse: the caller's torch.unique of cand_keys; masks zeroed by the caller); cand_keys
 * is sr_stsdf_touch's output for B <= 64 frames (n_cand = B * cand_per_frame, cand_per_frame = 8 S).
 *
 * Integration (fp32, no FMA contraction, in this order; sr_stsdf_integrate).  Each block of the call (slot >= 0)
 * applies the frames of its mask in ascending frame order, and no others; per voxel and frame f:
 *  - centre c = ((float)g + 0.5f) * vl per axis; p = R c + t row by row as ((r0 x + r1 y) + r2 z) + t; skip if
 *    p.z <= 0.
 *  - u_f = ((p.x * fx) / p.z + cx) + 0.5f, v_f likewise; skip unless 0.0001f <= u_f < w - 0.0001f and 0.0001f <= v_f
 *    < h - 0.0001f; u = (int)u_f, v = (int)v_f.  D = depth[v][u]; skip if D <= 0.
 *  - a = (u - cx) / fx, b = (v - cy) / fy, sdf = (D - p.z) * sqrtf((1 + a * a) + b * b) (correctly rounded sqrtf).
 *  - if sdf > -sdf_trunc (NaN fails): t' = min(1, sdf / sdf_trunc); tsdf = (tsdf * W + t') / (W + 1);
 *    rgb = (rgb * W + c) / (W + 1) per channel, c the pixel's uint8 colour (colour NULL: 178); W = W + 1.
 * frames [B][SR_STSDF_FRAME_FLOATS] fp32: R row-major [0,9), t [9,12), fx, fy, cx, cy [12,16) (cam_T_world and K).
 * color [B][3][h][w] uint8 or NULL.
 *
 * Mesh extraction (sr_stsdf_mesh_count, sr_stsdf_mesh_emit).  The rules of "mesh extraction" above, on the fp32 tsdf
 * (clamped to [-1, 1], not rounded through fp16), level 0, where a voxel with W == 0 or in an unallocated block is NaN.
 * Blocks in ascending key order (keys [n] sorted ascending, slots [n] their pool slots).  Vertices are numbered block
 * by block, then by l, then x, y, z edge; faces likewise by block, l, loop order.  Voxel-unit positions p use the
 * global g (exact while |g| < 2^24); vertex = (p + 0.5f) * vl; vertex colour = (c0 + t * (c1 - c0)) / 255 per channel,
 * c0 / c1 the rgb of the edge's lower / upper voxel and t the edge parameter.  No normals.
 * sr_stsdf_mesh_count writes block_counts [2][n] int32 (vertices, faces of each block).  The caller forms
 * block_offsets [2][n] int64, their exclusive prefix sums, and reads the totals; sr_stsdf_mesh_emit then writes
 * vertices [V,3] fp32, colors [V,3] fp32 and faces [F,3] int32, with vertex_table [n][3][4096] int32 as scratch.
 *
 * The library allocates nothing and no call synchronises with the host.  Only the touch masks use atomics (integer OR:
 * the result does not depend on the order), so every output is the same bits on every run.  Refused
 * (SR_ERR_INVALID_ARGUMENT): NULL required pointers, B outside [1, 64], h or w outside [1, 2^15], 2 sdf_trunc >= unit,
 * non-positive voxel_length or sdf_trunc, a slot outside [0, capacity). */
#define SR_STSDF_FRAME_FLOATS 16
#define SR_STSDF_MAX_FRAMES 64
#define SR_STSDF_KEY_NONE (-1ll)
int sr_stsdf_touch(const float* depth, int B, int h, int w, const double* frames_inv /* [B][16]: M rows 0..2, fx, fy,
                   cx, cy */, double sdf_trunc, double unit, int64_t* cand_keys, void* stream);
int sr_stsdf_block_masks(const int64_t* cand_keys, const int64_t* inverse, int64_t n_cand, int64_t cand_per_frame,
                         uint64_t* masks, void* stream);
int sr_stsdf_integrate(float* pool, int64_t capacity, const int64_t* block_keys, const int64_t* block_slots,
                       const uint64_t* block_masks, int64_t n_blocks, const float* frames, const float* depth,
                       const uint8_t* color, int B, int h, int w, float voxel_length, float sdf_trunc, void* stream);
int sr_stsdf_mesh_count(const float* pool, int64_t capacity, const int64_t* keys, const int64_t* slots, int64_t n_blocks,
                        int32_t* block_counts, void* stream);
int sr_stsdf_mesh_emit(const float* pool, int64_t capacity, const int64_t* keys, const int64_t* slots, int64_t n_blocks,
                       float voxel_length, const int64_t* block_offsets, int64_t num_vertices, int64_t num_faces,
                       int32_t* vertex_table, float* vertices, float* colors, int32_t* faces, void* stream);

/* ------------------------------------------------------------- mesh rasteriser ----
 *
 * Depth and face-id renders of one triangle mesh into B pinhole views (geometry only: no shading), and the per-face
 * visibility they give.  tests/raster_oracle.py is the float64 ray caster the renders are checked against.
 *
 * Inputs: vertices [V,3] fp32, faces [F,3] int32, K [B][16] and cam_T_world [B][16] fp32 row-major 4x4 (of K: fx =
 * K[0][0], fy = K[1][1], cx = K[0][2], cy = K[1][2]; skew is not supported), H, W <= SR_RASTER_MAX_SIDE, znear > 0,
 * pixel_offset o in [-1, 1].  Pixel (u, v) samples the ray ((u + o - cx) / fx, (v + o - cy) / fy, 1): o = 0 is this
 * project's backprojection convention, o = 0.5 OpenGL's pixel centres.
 *
 * Per (view, face), in fp64 from the fp32 inputs:
 *  - X = R x + t per vertex.  The face is dropped when an index is outside [0, V), when n = (X1 - X0) x (X2 - X0) is
 *    zero or not finite, or when the plane passes through the camera centre.  n is normalised, c = n . X0; the face
 *    is front-facing when c < 0 (n points at the camera centre; TriangleMesh's winding, counter-clockwise seen from
 *    free space).  SR_RASTER_CULL_BACK drops the others.
 *  - The triangle is clipped at z = znear / 2 (one triangle may become two; a cut point is always computed from the
 *    vertex in front to the vertex behind, so two faces sharing an edge share the point).  The clip only keeps the
 *    projection finite: the pixel test z >= znear below decides what is seen.
 *  - Projection x = fx X / Z + cx - o, y likewise: pixel centres are the integers.  The bounding box is clamped to the
 *    image; a box without a pixel centre, or a projected area of zero, drops the triangle.
 *  - Coverage: a pixel belongs to the triangle when it lies inside or on its three edges.  An edge's value is computed
 *    from its two end points in an order that depends on the points alone, so the two faces on a shared edge see
 *    exactly opposite values: a pixel is never missed by both.
 *  - Depth, fp32: z = c / ((n_x r_x + n_y r_y) + n_z) with r the pixel's ray above -- the camera-space plane along
 *    the ray, not interpolated screen-space z.  A pixel is hit when znear <= z < inf.
 * Each hit does atomicMin on the pixel's key (bits of z) << 32 | face: the image does not depend on the launch
 * order and equal depths go to the lowest face id.  Boxes of at most 256 pixels are walked by one lane of the setup
 * kernel; larger ones become records, are cut into tiles of 16 x 4 pixels, and one wave serves each (record, tile) --
 * no thread loops over more than 256 pixels.
 *
 * Use: sr_raster_small (sets keys [B,H,W] to empty and counters [2] to 0, draws the small triangles, counts the
 * large ones in counters[0]) -> if any: sr_raster_large_setup (records [capacity][SR_RASTER_RECORD_BYTES], 8-byte
 * aligned, and tile_counts [capacity] int32, capacity >= counters[0]; slots are taken from counters[1]) -> the
 * caller's inclusive prefix sum of tile_counts as int64 (tile_ends; its last entry is num_items) -> sr_raster_large
 * -> sr_raster_resolve (depth [n] fp32, 0 where empty; face [n] int32, -1 where empty; either may be NULL).
 *
 * Visibility.  sr_raster_visibility_mask sets bit b of masks[f] (uint64 [F], zeroed by the caller before the first
 * call) for every pixel of view b < B <= SR_RASTER_MASK_VIEWS that face f won.  sr_raster_visibility_count adds each
 * mask's bit count to counts [F] int32 (zeroed by the caller before the first call), clears the mask, and writes
 * visible[f] = counts[f] >= min_views (uint8, optional): more than 64 views go through in groups.
 *
 * Integer atomics only: every output is the same bits on every run.  The library allocates nothing and no call
 * synchronises with the host.  Refused (SR_ERR_INVALID_ARGUMENT): NULL required pointers, counts or sizes outside
 * their range (SR_RASTER_MAX_THREADS, SR_RASTER_MAX_PAIRS: render more views in several calls), an unknown cull mode, a misaligned record buffer. */
#define SR_RASTER_CULL_NONE 0
#define SR_RASTER_CULL_BACK 1
#define SR_RASTER_MAX_SIDE 32768
#define SR_RASTER_RECORD_BYTES 80
#define SR_RASTER_MASK_VIEWS 64
#define SR_RASTER_MAX_THREADS 0xffffff00ll /* per launch: B * H * W, B * F and 64 * num_items stay at or below it */
#define SR_RASTER_MAX_PAIRS (1ll << 30)    /* B * F: the int32 counters hold two triangles per (view, face) */
int sr_raster_small(const float* vertices, int64_t num_vertices, const int32_t* faces, int64_t num_faces, const float* K,
                    const float* cam_T_world, int B, int H, int W, float znear, float pixel_offset, int cull,
                    uint64_t* keys, int32_t* counters, void* stream);
int sr_raster_large_setup(const float* vertices, int64_t num_vertices, const int32_t* faces, int64_t num_faces,
                          const float* K, const float* cam_T_world, int B, int H, int W, float znear, float pixel_offset,
                          int cull, int64_t capacity, int32_t* counters, void* records, int32_t* tile_counts,
                          void* stream);
int sr_raster_large(const void* records, const int64_t* tile_ends, int64_t num_large, int64_t num_items, const float* K,
                    int B, int H, int W, float znear, float pixel_offset, uint64_t* keys, void* stream);
int sr_raster_resolve(const uint64_t* keys, int64_t n, float* depth, int32_t* face, void* stream);
int sr_raster_visibility_mask(const int32_t* face_bhw, int B, int64_t pixels_per_view, int64_t num_faces,
                              uint64_t* masks, void* stream);
int sr_raster_visibility_count(uint64_t* masks, int64_t num_faces, int32_t* counts, int min_views, uint8_t* visible,
                               void* stream);

/* ------------------------------------------------------------- mesh shading ----
 *
 * Colour and shaded renders of a mesh from the face-id image sr_raster_resolve writes (a deferred pass), and the
 * vertex normals that pass needs.  tests/shade_oracle.py restates both in float64 numpy; that file is the yardstick.
 * The shading model is a stated one, ambient plus Lambert: pyrender, whose metallic-roughness shader the reference
 * draws with, cannot be run next to this code, and nothing here tries to match its pictures (the same standing as the
 * half-pixel convention of the rasteriser, simplerecon_amd/render.py).
 *
 * sr_mesh_vertex_normals: area-weighted vertex normals (Open3D's compute_vertex_normals rule),
 *     n_v = normalise(sum over the faces f that contain v of (x1 - x0) x (x2 - x0)),
 * summed in fp64 from the fp32 vertices in ascending face order, normals [V,3] fp32.  A face is skipped when one of
 * its indices is outside [0, V) or its cross product is not finite.  A vertex gets (0, 0, 0) when no usable face
 * touches it or when its sum is zero or not finite.  The caller sorts the 3F face corners (corner 3f + j is vertex j
 * of face f) by vertex id with a STABLE sort: corner_order [3F] int64 is that permutation, vertex_offsets [V + 1]
 * int64 the start of every vertex's run in it (corners whose vertex id is outside [0, V) sort behind the last
 * run).  One thread sums one vertex's run, so there is no atomic and the result is the same bits on every run.  Entries
 * of the two arrays that point outside the faces, or at a corner that is not the vertex's, are ignored.
 *
 * sr_raster_shade: mesh, K, cam_T_world, H, W and pixel_offset as for the rasteriser; face_bhw [B,H,W] int32 (-1, or
 * any value outside [0, F), or a face with an index outside [0, V): an empty pixel); colors [V,3] fp32 or NULL; normals
 * [V,3] fp32 (world frame) or NULL.  HOST arrays, read before the call returns: base_color [3], background [3], lights
 * [num_lights][SR_SHADE_LIGHT_FLOATS] = (kind, x, y, z, r, g, b intensity, unused), num_lights <= SR_SHADE_MAX_LIGHTS.
 * Per pixel with a face, in fp64 from the fp32 inputs, every step a separately rounded IEEE operation (correctly
 * rounded divide and square root, no fused multiply-add), rounded to fp32 once at the end:
 *  - X_i = R x_i + t; a = X_0, e1 = X_1 - X_0, e2 = X_2 - X_0, n = e1 x e2; the pixel's ray r as the rasteriser
 *    defines it; d = r . n; hit point P = ((a . n) / d) r.  Barycentrics from the ray (perspective-correct, and valid
 *    for a face the rasteriser clipped): u = -(r . (a x e2)) / d, v = -(r . (e1 x a)) / d, w = (1 - (u + v), u, v), each
 *    clamped to [0, 1], then divided by their sum.  An attribute is interpolated as x_0 w_0 + (x_1 w_1 + x_2 w_2).
 *  - base colour c: the interpolated vertex colour, or base_color without colours.
 *  - geometric normal n_g = n / |n|, negated when n_g . P > 0 (it faces the viewer).  Smooth normal: m = R (the
 *    interpolated vertex normal), n = m / |m|, negated when the face is back-facing (a . n >= 0, the rasteriser's
 *    rule); n = n_g when |m| < 1e-12 or is not finite, without normals, and with SR_SHADE_NORMAL_FLAT.
 *  - SR_SHADE_UNLIT: out = c.  SR_SHADE_NORMALS: out = 0.5 (1 + n), n in the camera frame.  SR_SHADE_LAMBERT:
 *    out_k = c_k (ambient + sum_l I_lk max(0, n . l_l) a_l), where max(0, NaN) = 0 and per kind
 *      SR_SHADE_LIGHT_DIRECTIONAL  xyz = the direction the light travels, world frame: l = -R (xyz / |xyz|), a = 1
 *      SR_SHADE_LIGHT_POINT        xyz = the position, world frame: with D = (R xyz + t) - P, l = D / |D|,
 *                                  a = 1 / max(|D|^2, 1e-12)
 *      SR_SHADE_LIGHT_HEAD         l = -P / |P|, a = 1
 * Outputs, any of them NULL but not all: out_f32 [B,3,H,W] clamped to [0, 1] with NaN -> 0; out_u8 [B,H,W,3]
 * interleaved = (uint8)(out_f32 * 255.0f) truncated, in fp32 from the value out_f32 holds (sr_viz's rule);
 * normals_out [B,3,H,W] = n, 0 where the pixel is empty.  An empty pixel gets `background` as given in out_f32 (and
 * its bytes by the same rule, clamped).
 *
 * A workgroup owns 256 consecutive pixels of one view, one lane each; B * ceil(H W / 256) * 256 must stay within
 * SR_RASTER_MAX_THREADS.  All offsets are 64-bit; no atomics; the library allocates nothing and no call synchronises
 * with the host.  Refused on the host before any launch (SR_ERR_INVALID_ARGUMENT): NULL required pointers, no output,
 * an unknown shading mode, normal mode or light kind, more than SR_SHADE_MAX_LIGHTS lights, sizes beyond
 * SR_RASTER_MAX_SIDE or SR_RASTER_MAX_THREADS, a pixel_offset outside [-1, 1]. */
#define SR_SHADE_UNLIT 0
#define SR_SHADE_NORMALS 1
#define SR_SHADE_LAMBERT 2
#define SR_SHADE_NORMAL_SMOOTH 0
#define SR_SHADE_NORMAL_FLAT 1
#define SR_SHADE_LIGHT_DIRECTIONAL 0
#define SR_SHADE_LIGHT_POINT 1
#define SR_SHADE_LIGHT_HEAD 2
#define SR_SHADE_MAX_LIGHTS 32
#define SR_SHADE_LIGHT_FLOATS 8
int sr_mesh_vertex_normals(const float* vertices, int64_t num_vertices, const int32_t* faces, int64_t num_faces,
                           const int64_t* corner_order, const int64_t* vertex_offsets, float* normals, void* stream);
int sr_raster_shade(const float* vertices, int64_t num_vertices, const int32_t* faces, int64_t num_faces, const float* K,
                    const float* cam_T_world, int B, int H, int W, float pixel_offset, const int32_t* face_bhw,
                    const float* colors, const float* normals, const float* base_color, const float* background,
                    float ambient, const float* lights, int num_lights, int shading, int normal_mode, float* out_f32,
                    uint8_t* out_u8, float* normals_out, void* stream);

/* ------------------------------------------------------------- frame preparation ----
 *
 * What the reference's data loader does to a decoded frame (datasets/generic_mvs_dataset.py get_frame,
 * utils/generic_utils.py read_image_file): Pillow's Image.resize of the 8-bit colour image, to_tensor + ImageNet
 * normalisation, and the nearest resize of the 16-bit depth map with its validity masks -- reproduced bit for bit.
 * simplerecon_amd/frames.py builds the tables on the host (the only place the Pillow rules below are coded);
 * tests/frames_oracle.py restates the kernels in numpy.
 *
 * Colour resize, 8 bits per channel, `in` uint8 [B,h,w,C] interleaved, C in 1..4, every channel on its own (an RGBA
 * image is NOT premultiplied: Pillow's result for CMYK / RGBX, not for RGBA).  Pillow runs a horizontal pass, rounds
 * it to uint8, then runs a vertical pass; a pass whose size does not change is skipped (here: an identity table,
 * one tap of weight 2^22, which copies).  Per output index i of a pass, with scale = in / out, fs = max(scale, 1),
 * support = filter support * fs and centre = (i + 0.5) * scale: taps first = int(centre - support + 0.5) clamped at 0
 * to last = int(centre + support + 0.5) clamped at `in`; weight of tap x = filter((x - centre + 0.5) / fs), normalised
 * by their sum in double, then k = int(w * 2^22 +- 0.5) (sign of w).  Output = clamp((2^21 + sum k * v) >> 22, 0, 255)
 * in wrapping 32-bit integers.
 * A table holds out * (2 + taps) int32: per output index [first, count, k_0 .. k_(taps-1)], count <= taps, unused
 * weights 0.  The kernels trust it: first >= 0 and first + count <= in for every entry.
 *
 * sr_frames_resize writes `out` uint8 [B,H,W,C] (f32_out = 0), or fp32 planes [B,C,H,W] = lut[c][value] (f32_out = 1;
 * lut [C][256]: ((v / 255) - mean_c) / std_c as torch's CPU kernels round it, computed by the caller), columns
 * mirrored when flip.  lds_rows > 0: ONE launch -- a workgroup owns SR_FRAMES_TILE_H output rows x
 * SR_FRAMES_TILE_W output columns, resamples horizontally the input rows they tap into LDS (uint8 [lds_rows]
 * [SR_FRAMES_TILE_W * C]) and vertically from there; lds_rows must be at least the largest number of input rows any
 * SR_FRAMES_TILE_H consecutive output rows tap (last tap of the last row - first tap of the first), and
 * sr_frames_resize_fits_lds(C, x_taps, lds_rows, f32_out) must hold (tables and rows within SR_FRAMES_LDS_BYTES).
 * lds_rows = 0: two launches through `tmp` uint8 [B,h,W,C] (very large downscale factors).  Both give the same bytes.
 *
 * sr_frames_depth: `in` [B,h,w] uint16 (in_is_int32 = 0) or int32 with values 0..65535; ysrc [H] / xsrc [W] int32
 * source indices (Pillow's nearest: floor((i + 0.5) * in / out) in double; the identity for the native size),
 * trusted to lie inside the input.  d = float(v) * scale in fp32; valid = (d > min_valid) & (d < max_valid) with both
 * bounds rounded to fp32, as torch compares an fp32 tensor with a Python scalar.  Writes depth [B,1,H,W] (NaN where
 * invalid), mask (1.0 / 0.0) and mask_b (uint8 1 / 0), columns mirrored when flip.
 *
 * All offsets are 64-bit.  SR_ERR_UNSUPPORTED: a side above SR_FRAMES_MAX_SIDE, B above SR_FRAMES_MAX_BATCH, C outside
 * 1..4, an lds_rows that does not fit.  No call allocates or synchronises with the host. */
#define SR_FRAMES_TILE_W 128
#define SR_FRAMES_TILE_H 16
#define SR_FRAMES_LDS_BYTES 49152
#define SR_FRAMES_MAX_SIDE 32768
#define SR_FRAMES_MAX_BATCH 65535
int sr_frames_resize_fits_lds(int C, int x_taps, int lds_rows, int f32_out);
int sr_frames_resize(const uint8_t* in, int B, int h, int w, int C, const int32_t* xtab, int x_taps, const int32_t* ytab,
                     int y_taps, int lds_rows, const float* lut, void* out, int f32_out, int H, int W, int flip,
                     uint8_t* tmp, void* stream);
int sr_frames_depth(const void* in, int in_is_int32, int B, int h, int w, const int32_t* ysrc, const int32_t* xsrc, int H,
                    int W, float scale, float min_valid, float max_valid, int flip, float* depth, float* mask,
                    uint8_t* mask_b, void* stream);

/* Colour jitter: transforms.ColorJitter on the to_tensor image, which the reference's loader runs on every frame of a
 * training tuple before the flip and the normalisation (generic_mvs_dataset.py:517-525, ColorJitter(0.2, 0.2, 0.2,
 * 0.2)).  torchvision is not a dependency of this library and is absent where it was written: what follows restates
 * the published tensor path (ColorJitter.forward, functional_tensor) and PARITY AGAINST THE PACKAGE ITSELF IS UNPINNED.
 * tests/jitter_oracle.py is the same rule in torch's CPU operations.
 *
 * Input: the resized 8-bit image uint8 [B,H,W,3] interleaved (what sr_frames_resize writes), x = float(v) / 255.0f per
 * channel.  Every operation below is a separately rounded fp32 operation (no fused multiply-add, correctly rounded
 * division), in the order written.
 *     gray(x)        = 0.2989 r + 0.587 g + 0.114 b
 *     blend(a, b, f) = clamp(f a + (1 - f) b, 0, 1); 1 - f is computed by the host in double and passed as a second fp32
 *                      number, as torch passes a Python scalar.  Every operator ends in this clamp.
 *     0 brightness   blend(x, 0, f) = clamp(f x)
 *     1 contrast     blend(x, m, f), m = the mean over all pixels of gray(x) of the image as it stands when the
 *                    operator runs (summed in double here, divided by H W in double, rounded to fp32)
 *     2 saturation   blend(x, gray(x), f) per pixel
 *     3 hue          rgb2hsv, h = (h + f) mod 1 with Python's sign convention, hsv2rgb:
 *         rgb2hsv: maxc / minc over the channels; eq = maxc == minc; cr = maxc - minc; s = cr / (eq ? 1 : maxc);
 *                  d = eq ? 1 : cr; (rc, gc, bc) = (maxc - (r, g, b)) / d;
 *                  h' = (maxc == r) ? bc - gc : (maxc == g) ? 2 + rc - bc : 4 + gc - rc;
 *                  h = fmod(h' / 6 + 1, 1); v = maxc
 *         hsv2rgb: i = floor(6 h); fr = 6 h - i; i = i mod 6; p = clamp(v (1 - s)); q = clamp(v (1 - s fr));
 *                  t = clamp(v (1 - s (1 - fr))); rgb = (v,t,p), (q,v,p), (p,v,t), (p,q,v), (t,p,v), (v,p,q) for i = 0..5
 *         (a mod 1 is a - floor(a): the shifted hue of a slightly negative sum rounds to 1.0, which hsv2rgb takes as 0)
 * The rule is continuous across hue sectors, ties of the largest channel and greys.
 *
 * Parameters (ColorJitter.__init__ / get_params; drawn by simplerecon_amd/frames.py jitter_params): a value a for
 * brightness, contrast or saturation means the range [max(0, 1 - a), 1 + a], for hue [-a, a] with 0 <= a <= 0.5; a
 * (lo, hi) pair is taken as given; a range that collapses to the neutral value switches the operator off, and an
 * operator that is off is neither drawn nor applied.  One draw per frame: order = randperm(4), then for each operator
 * that is on, in the order brightness, contrast, saturation, hue, one uniform_(lo, hi) as fp32; the operators run in
 * `order`.  The loader draws the flip once per tuple first, then the jitter of each frame, the reference frame first.
 *
 * Table `params`, on the device, SR_FRAMES_JITTER_PARAM_WORDS 32-bit words per frame: [0..3] int32 operator ids in the
 * order they run, -1 for an empty slot; then fp32 [4] brightness f, [5] 1 - f, [6] contrast f, [7] 1 - f,
 * [8] saturation f, [9] 1 - f, [10] hue shift, [11] unused.  The kernels trust it: sr_frames_jitter_check_params reads
 * the HOST copy before it is sent and returns SR_ERR_INVALID_ARGUMENT for an id outside -1..3 or an operator that
 * appears twice in a frame; a kernel passes over a slot it does not know.
 *
 * sr_frames_jitter writes `out` fp32 planes [B,3,H,W], columns mirrored when flip, (x - mean_c) / std_c with the
 * ImageNet constants rounded to fp32 when normalise (a rounded subtract, then a rounded divide: to_tensor + normalize
 * of an image with no operator on gives the bytes of sr_frames_resize's f32 output).  Two launches:
 *   mean pass   only when `scratch` is given.  Workgroup x of frame b applies the operators in front of contrast to
 *               its pixels, adds their grey in double (registers, wave butterfly, LDS) and writes partial [b][x]; at
 *               most SR_FRAMES_JITTER_MAX_PARTIALS workgroups per frame, each striding over the frame.  A frame
 *               without contrast leaves at once.
 *   apply pass  adds the frame's partials in one fixed tree (no atomics: equal bytes on every run), recomputes the
 *               whole chain per pixel, flips, normalises, stores.  A lane owns 4 consecutive pixels of a row: when
 *               W % 4 == 0, `in_u8` is 4-byte and `out` 16-byte aligned it loads three words and stores 16 bytes per
 *               plane (with flip, its four pixels reversed); otherwise it moves single bytes and floats, the last
 *               lane of a row fewer than four.
 * scratch = NULL says no frame has contrast on: the mean pass is not launched and a contrast slot is passed over.
 * Otherwise scratch is 8-byte aligned with at least sr_frames_jitter_scratch_bytes(B, H, W) bytes
 * (SR_ERR_WORKSPACE_TOO_SMALL).  Both passes read 3 bytes per pixel and the apply pass writes 12: 18 bytes per pixel.
 * All offsets are 64-bit.  SR_ERR_UNSUPPORTED: a side above SR_FRAMES_MAX_SIDE, B above SR_FRAMES_MAX_BATCH.  No
 * call allocates or synchronises with the host; both launches can be captured in a HIP graph. */
#define SR_FRAMES_JITTER_PARAM_WORDS 12
#define SR_FRAMES_JITTER_MAX_PARTIALS 128
#define SR_FRAMES_JITTER_BRIGHTNESS 0
#define SR_FRAMES_JITTER_CONTRAST 1
#define SR_FRAMES_JITTER_SATURATION 2
#define SR_FRAMES_JITTER_HUE 3
size_t sr_frames_jitter_scratch_bytes(int B, int H, int W);
int sr_frames_jitter_check_params(const void* params_host, int B);
int sr_frames_jitter(const uint8_t* in_u8, int B, int H, int W, const void* params, float* out, int flip, int normalise,
                     void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------ visualisation ----
 *
 * The pictures the reference makes with utils/visualization_utils.py (colormap_image, quick_viz_export) and its
 * training log (experiment_modules/depth_model.py:542-562), computed where the maps already are.  An image is n = H * W
 * fp32 values, a batch B images back to back.  Every pixel value is a chain of separately rounded IEEE fp32 operations
 * in the order written below (correctly rounded division, no fused multiply-add), so results equal the reference's CPU
 * results bit for bit.
 *
 * Masks: mask_kind SR_VIZ_MASK_NONE (mask ignored), SR_VIZ_MASK_U8 (uint8 / bool [B,n]) or SR_VIZ_MASK_F32 (fp32
 * [B,n]).  A value is SELECTED where the mask is non-zero (Tensor.bool(): NaN and -1 select, -0.0 does not); the mask's
 * float VALUE m (1 / 0 for 8-bit masks) blends colours.
 *
 * sr_viz_range: minimum and maximum of the selected values, range [B,2] = (min, max) per image, or [2] over the whole
 * batch when pooled.  One selected NaN makes both ends NaN (torch.min / torch.max).  An EMPTY selection gives NaN for
 * both ends: the reference raises there, which cannot be done without a host synchronisation (a documented departure).
 * Min and max do not depend on the order of comparisons (-0 orders below +0), so the result is the same bits on every
 * run.  Two launches through `workspace` (sr_viz_range_workspace_bytes, 4-byte aligned); the result stays on the
 * device.
 *
 * sr_viz_colormap, per pixel x of image b:
 *     t = (x - vmin) / (vmax - vmin);  i = (int) clamp(t * 255, 0, 255), truncated toward zero, NaN -> 0
 *     rgb = lut[i]                                 lut: [256,3] fp32 (already reversed by the caller for flip=True)
 *     with a mask: rgb = rgb * m + invalid * (1 - m)
 * vmin = vmin_dev[b * vmin_stride] when vmin_dev is not NULL (stride 2 into a [B,2] range, 0 for a shared value), else
 * the host scalar `vmin`; vmax likewise.  Writes out_f32 [B,3,n] (the reference's result), out_u8 [B,n,3] interleaved
 * = (uint8) clamp(rgb * 255, 0, 255) truncated (np.uint8(rgb * 255); the clamp changes nothing in range, NaN -> 0),
 * or both; at least one must be given.
 *
 * sr_viz_unit: `in` [B,3,n] fp32 -> the same two outputs, with v =
 *     SR_VIZ_UNIT_NORMALS  nan_to_num(0.5 * (1 + x))           (NaN -> 0, +-inf -> +-FLT_MAX)
 *     SR_VIZ_UNIT_COLOR    (x - mean_c) / std_c                utils/generic_utils.py reverse_imagenet_normalize:
 *                          mean = (-2.11790393, -2.03571429, -1.80444444), std = (4.36681223, 4.46428571, 4.44444444),
 *                          rounded to fp32; subtract then divide (torchvision's normalize)
 * Values that leave [0, 1] are clamped in the 8-bit output (np.uint8 of an out-of-range float is undefined).
 *
 * A workgroup owns SR_VIZ_CHUNK consecutive pixels of one image.  When n % 4 == 0 and every array is 16-byte aligned
 * (4 bytes for 8-bit arrays) a thread moves 4 pixels per access, otherwise 1: same values either way.  All offsets are
 * 64-bit.  SR_ERR_UNSUPPORTED: B above SR_VIZ_MAX_BATCH, n above SR_VIZ_MAX_PIXELS.  No call allocates or
 * synchronises with the host. */
#define SR_VIZ_MASK_NONE 0
#define SR_VIZ_MASK_U8 1
#define SR_VIZ_MASK_F32 2
#define SR_VIZ_UNIT_NORMALS 0
#define SR_VIZ_UNIT_COLOR 1
#define SR_VIZ_CHUNK 4096
#define SR_VIZ_MAX_BATCH 65535
#define SR_VIZ_MAX_PIXELS (1ll << 30)
size_t sr_viz_range_workspace_bytes(int B, int64_t n);
int sr_viz_range(const float* image, const void* mask, int mask_kind, int B, int64_t n, int pooled, float* range,
                 void* workspace, size_t workspace_bytes, void* stream);
int sr_viz_colormap(const float* image, const void* mask, int mask_kind, int B, int64_t n, const float* lut,
                    const float* vmin_dev, int64_t vmin_stride, const float* vmax_dev, int64_t vmax_stride, float vmin,
                    float vmax, float invalid_r, float invalid_g, float invalid_b, float* out_f32, uint8_t* out_u8,
                    void* stream);
int sr_viz_unit(const float* in, int B, int64_t n, int mode, float* out_f32, uint8_t* out_u8, void* stream);

/* ------------------------------------------------------ backward (training) -------------
 *
 * Backward of sr_dot_volume_sweep (reference: autograd through CostVolumeManager.build_cost_volume,
 * modules/cost_volume.py:237-335 -- grid_sample backward + the broadcasting mul / sum): given grad_cv = dL/d
 * cost_volume (strides g_sb, g_sd, g_sp like the forward's volume strides), writes d_cur [B,C,h,w] and / or
 * d_src [B,K,C,h,w] (either may be NULL).  Poses, intrinsics and depth planes are data (no gradient, as in the
 * reference).  `workspace` must have been filled by sr_volume_prepare for the same src / K_src / T_src_cur (what
 * sr_dot_volume_fwd leaves behind); `scratch` (sr_dot_volume_bwd_scratch_bytes, 16-byte aligned) holds the
 * channels-last d_src accumulation image.  d_src is accumulated with hardware fp32 atomics: its summation order, like
 * torch's grid_sample backward, is not fixed. */
size_t sr_dot_volume_bwd_scratch_bytes(int B, int K, int C, int h, int w);
int sr_dot_volume_bwd(const float* grad_cv, int64_t g_sb, int64_t g_sd, int64_t g_sp, const float* cur,
                      const float* invK_cur, const float* planes, int64_t ps_b, int64_t ps_d, int64_t ps_y,
                      int64_t ps_x, int B, int K, int C, int h, int w, int D, float* d_cur, float* d_src,
                      void* workspace, size_t workspace_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* ---- backward of the conv stack (reference: autograd through BasicBlock / CVEncoder / DepthDecoderPP, modules/layers.py:
 * 24-85, modules/networks.py:20-127; train.py:126-145).  Data gradients reuse the forward kernels on
 * sr_conv_flip_transpose_weights(W) (stride 2: on the sr_zero_stuff2x_nhwc'ed output gradient).
 *  sr_conv_wgrad_nhwc            d_weight [Cout,Cin,k,k] (written, not accumulated) = sum over pixels of grad_out x input
 *                                patches; fp32 MFMA, per-workgroup partial slabs in `workspace`
 *                                (sr_conv_wgrad_workspace_bytes) added in index order by a second kernel (deterministic)
 *  sr_bias_grad_nhwc             d_bias [C] = sum over pixels of grad_out
 *  sr_act_bwd                    grad * LeakyReLU'(saved output), dense arrays of n floats
 *  sr_act_bwd_bias_nhwc          both of the above in one float4 pass over a dense [pixels, C] gradient (C % 4 == 0):
 *                                grad_pre = grad * LeakyReLU'(out_saved) (out_saved null: no activation, nothing written),
 *                                d_bias = sum over pixels of grad_pre (null: skipped); per-block partial sums in
 *                                `workspace` (sr_act_bwd_bias_workspace_bytes) are added in block order (deterministic)
 *  sr_zero_stuff2x_nhwc          out [B,Hs,Ws,C] dense: out[:, 2y, 2x] = in[:, y, x], zero elsewhere
 *  sr_upsample2x_bwd_nhwc        adjoint of sr_upsample2x_nhwc_fwd: grad_out [B,2H,2W,C] -> grad_in [B,H,W,C]
 *  sr_conv_flip_transpose_weights  out [Cin,Cout,k,k] = W[co,ci,k-1-ky,k-1-kx]
 *  sr_mul_fwd                    out = a * b (backward of depth = exp(log_depth)) */
size_t sr_conv_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout, int ksize, int stride);
int sr_conv_wgrad_nhwc(const float* in, int64_t in_batch_stride, int in_pix_stride, const float* grad_out,
                       int64_t g_batch_stride, int g_pix_stride, float* d_weight, int B, int H, int W, int Cin, int Cout,
                       int ksize, int stride, void* workspace, size_t workspace_bytes, void* stream);
int sr_bias_grad_nhwc(const float* grad_out, int64_t g_batch_stride, int g_pix_stride, float* d_bias, int B, int H, int W,
                      int C, void* stream);
int sr_act_bwd(const float* grad, const float* out_saved, float* grad_pre, int64_t n, float leaky_slope, void* stream);
size_t sr_act_bwd_bias_workspace_bytes(int64_t pixels, int C);
int sr_act_bwd_bias_nhwc(const float* grad, const float* out_saved, float* grad_pre, float* d_bias, int64_t pixels, int C,
                         float leaky_slope, void* workspace, size_t workspace_bytes, void* stream);
int sr_zero_stuff2x_nhwc(const float* in, int64_t in_batch_stride, int in_pix_stride, float* out, int B, int H, int W,
                         int Hs, int Ws, int C, void* stream);
int sr_upsample2x_bwd_nhwc(const float* grad_out, int64_t g_batch_stride, int g_pix_stride, float* grad_in,
                           int64_t in_batch_stride, int in_pix_stride, int B, int H, int W, int C, void* stream);
int sr_conv_flip_transpose_weights(const float* weight, int Cout, int Cin, int ksize, float* out, void* stream);
int sr_mul_fwd(const float* a, const float* b, float* out, int64_t n, void* stream);

/* Backward of sr_mlp_volume_sweep (reference: autograd through FeatureVolumeManager.build_cost_volume + MLP,
 * modules/cost_volume.py:451-736, modules/networks.py:129-147): d_cur [B,C,h,w], d_src [B,K,C,h,w] and the gradients
 * of the six MLP tensors in their nn.Linear layouts (dW1 [hidden][Cin], db1, dW2 [hidden][hidden], db2, dW3 [1][hidden],
 * db3 [1]; all written, not accumulated).  W1..W3 are the UNPACKED nn.Linear weights.  `workspace` must have been filled
 * by sr_volume_prepare WITH T_cur_src (pose features) for the same sources; `scratch`
 * (sr_mlp_volume_bwd_scratch_bytes, 256-byte aligned) holds the channels-last d_src image and weight transposes.
 * hidden = 128, C = 16, up to 15 views (MLP width <= 416); SR_ERR_UNSUPPORTED otherwise.  The six GEMM-shaped phases run on
 * the fp32 matrix cores (v_mfma_f32_32x32x2_f32).
 * Feature-map and weight gradients are accumulated with hardware fp32 atomics (summation order not fixed). */
size_t sr_mlp_volume_bwd_scratch_bytes(int B, int K, int C, int h, int w, int hidden);
int sr_mlp_volume_bwd(const float* grad_cv, int64_t g_sb, int64_t g_sd, int64_t g_sp, const float* cur,
                      const float* invK_cur, const float* planes, int64_t ps_b, int64_t ps_d, int64_t ps_y,
                      int64_t ps_x, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3,
                      float leaky_slope, int B, int K, int C, int h, int w, int D, int hidden, float* d_cur,
                      float* d_src, float* dW1, float* db1, float* dW2, float* db2, float* dW3, float* db3,
                      void* workspace, size_t workspace_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------ image-prior encoder ------------
 *
 * timm `tf_efficientnetv2_s` feature pyramid (reference modules/depth_model.py:110-116: the `encoder` of
 * DepthModel; third-party architecture).  Dense convolutions (stem, ConvBnAct, FusedMBConv, every 1x1) use
 * sr_conv2d_padded_nhwc_fwd / sr_conv2d_nhwc_fwd with eval-mode BatchNorm folded into weight and bias and
 * SR_ACT_SILU; the entry points below cover the depthwise / squeeze-excite part of the MBConv blocks.
 * All tensors channels-last fp32, C % 4 == 0, 16-byte aligned. */

/* Depthwise 3x3 convolution + bias + activation (`leaky_slope` as above).  weight9c: [9][C] tap-major
 * (= nn.Conv2d(C, C, 3, groups=C).weight[c, 0, ky, kx] at [(ky * 3 + kx) * C + c], BatchNorm scale folded in).
 * pool_partial (optional): [B][sr_dwconv3x3_pool_bands(Ho)][C] sums of the activated output over bands of
 * output rows -- the squeeze-excite average pool, finished by sr_se_gate_fwd. */
int sr_dwconv3x3_pool_bands(int Ho);
int sr_dwconv3x3_nhwc_fwd(const float* in, int64_t in_batch_stride, int in_pix_stride, const float* weight9c,
                          const float* bias, float* out, int64_t out_batch_stride, int out_pix_stride,
                          float* pool_partial, int B, int H, int W, int C, int stride, int pad_top, int pad_left,
                          int pad_bottom, int pad_right, float leaky_slope, void* stream);

/* Squeeze-excite gate: gate[b, c] = sigmoid(w_expand[c, :] . silu(w_reduce . mean[b, :] + b_reduce) + b_expand[c])
 * with mean[b, c] = (sum over bands of pool_partial[b, band, c]) / pixels.  w_reduce: [rd][C]; w_expand: [C][rd]. */
int sr_se_gate_fwd(const float* pool_partial, int bands, int pixels, const float* w_reduce, const float* b_reduce,
                   const float* w_expand, const float* b_expand, float* gate, int B, int C, int rd, void* stream);

/* EfficientNetV2's RGB stem (conv_stem of timm's tf_efficientnetv2_s, reference depth_model.py:110-116): act(conv3x3 /
 * stride 2 (3 -> 24) + bias) with explicit top / left zero padding (TF-"SAME": 0 / 0 on even images, the odd pixel goes
 * below / right), image read through its strides (NCHW or channels-last), output channels-last.  `weight27c` =
 * [ky][kx][ci][24] with the eval-mode BatchNorm scale folded in.  Byte work (29 MB in, 59 MB out per 8 images): a VALU
 * kernel, not the padded-K implicit GEMM.  Cout = 24 only (SR_ERR_UNSUPPORTED otherwise -> sr_conv2d_padded_nhwc_fwd). */
int sr_rgb_stem3x3s2_fwd(const float* image, int64_t sb, int64_t sc, int64_t sy, int64_t sx, const float* weight27c,
                         const float* bias, float* out, int64_t out_batch_stride, int out_pix_stride, int B, int H, int W,
                         int Cout, int pad_top, int pad_left, int Ho, int Wo, float act_code, void* stream);

/* The squeeze-excite gates alone, gate[b][c] = sigmoid(W2 silu(W1 mean_b + b1) + b2)[c], from sr_dwconv3x3_nhwc_fwd's partial
 * sums (timm SqueezeExcite of the MBConv blocks, reference depth_model.py:110-116) for a consumer that applies them itself:
 * sr_pw_conv_nhwc_fwd(gate = ...) scales the projection's input while loading it.  `hidden`: scratch [B][rd]. */
int sr_se_gate2_fwd(const float* pool_partial, int bands, int pixels, const float* w_reduce, const float* b_reduce,
                    const float* w_expand, const float* b_expand, float* hidden, float* gate, int B, int C, int rd,
                    void* stream);

/* The whole squeeze-excite step of an MBConv block in two short launches: hidden[b, j] = silu(w_reduce[j] . mean[b]
 * + b_reduce[j]) (workspace `hidden`: B * rd floats), then out[b, y, x, c] = in[b, y, x, c] * gate[b, c] with the gate
 * of sr_se_gate_fwd (also written to `gate` [B][C] when non-null).  rd <= 256; in-place allowed. */
int sr_se_scale_nhwc_fwd(const float* pool_partial, int bands, const float* w_reduce, const float* b_reduce,
                         const float* w_expand, const float* b_expand, float* hidden, const float* in,
                         int64_t in_batch_stride, int in_pix_stride, float* out, int64_t out_batch_stride,
                         int out_pix_stride, float* gate, int B, int H, int W, int C, int rd, void* stream);

/* out = a + b on channels-last views (in-place allowed): the identity skip of the stage-0 ConvBnAct blocks. */
int sr_add_nhwc_fwd(const float* a, int64_t a_batch_stride, int a_pix_stride, const float* b, int64_t b_batch_stride,
                    int b_pix_stride, float* out, int64_t out_batch_stride, int out_pix_stride, int B, int H, int W,
                    int C, void* stream);

/* out[b, y, x, c] = in[b, y, x, c] * gate[b, c] (in-place allowed). */
int sr_scale_channels_nhwc_fwd(const float* in, int64_t in_batch_stride, int in_pix_stride, const float* gate,
                               float* out, int64_t out_batch_stride, int out_pix_stride, int B, int H, int W, int C,
                               void* stream);

/* ------------------------------------------------------ encoder training path -----------
 *
 * Backward (and training-mode forward) pieces of the two encoders, csrc/sr_train.hip: the reference trains
 * ResnetMatchingEncoder (modules/networks.py:149-205) and the timm EfficientNetV2-S pyramid (depth_model.py:110-116) end
 * to end with BatchNorm in training mode (train.py:126-145).  Channels-last fp32 views (batch stride, pixel stride);
 * `act_code` as `leaky_slope` above (>= 0 LeakyReLU slope, SR_ACT_NONE, SR_ACT_SILU; SR_ACT_SIGMOID for the small dense
 * layers).  Column reductions are two-stage and deterministic (no atomics).
 *
 *  sr_norm_stats_nhwc        mean / biased variance per (group, channel) over pixels; per_image = 0: one group = the whole
 *                            batch (BatchNorm2d training statistics), 1: one group per image (InstanceNorm2d)
 *  sr_norm_act_fwd_nhwc      y = act(gamma * (x - mean) / sqrt(var + eps) + beta); gamma / beta [C] or null
 *  sr_norm_act_bwd_nhwc      dx (+ d_gamma, d_beta [C] when non-null); train_stats = 1: the statistics are functions of x
 *  sr_rowsum_nhwc            out[b, c] = scale * sum over pixels of x (g null) or of x * g
 *  sr_maxblurpool_bwd_nhwc   adjoint of sr_maxblurpool_nhwc_fwd (first maximum of a window receives its gradient)
 *  sr_replicate_pad_nhwc_fwd / _bwd   y [B,H+2p,W+2p,C] dense <- x clamped at the borders; adjoint (dense in / out)
 *  sr_im2col7x7s2_nhwc       col [B,Ho,Wo,Kp] of the 7x7 / stride-2 / pad-3 stem over a strided 3-channel image: with
 *                            sr_conv_wgrad_nhwc (1x1) it yields the stem's weight gradient
 *  sr_dwconv3x3_bwd_nhwc     depthwise 3x3 (weight [C][3][3], explicit top / left pad): d_in dense and / or d_weight
 *  sr_scale_bwd_nhwc         d_in = grad_out * gate[b, c] (+ pool_scale * d_pool[b, c]): backward of the squeeze-excite scaling
 *  sr_small_linear_fwd / _bwd   y = act(x W^T + b) on [B, K] -> [B, N] (the two dense layers of squeeze-excite)
 *  sr_act_in_bwd             grad * act'(saved input)
 *  sr_conv_wgrad_padded_nhwc sr_conv_wgrad_nhwc with explicit top / left zero padding and gradient size Ho x Wo */
#define SR_ACT_SIGMOID (-3.0f)
size_t sr_norm_workspace_bytes(int B, int HW, int C, int per_image);
int sr_norm_stats_nhwc(const float* x, int64_t x_batch_stride, int x_pix_stride, int B, int HW, int C, int per_image,
                       float* mean, float* var, void* workspace, size_t workspace_bytes, void* stream);
int sr_norm_act_fwd_nhwc(const float* x, int64_t x_batch_stride, int x_pix_stride, const float* mean, const float* var,
                         float eps, const float* gamma, const float* beta, float act_code, int per_image, float* y,
                         int64_t y_batch_stride, int y_pix_stride, int B, int HW, int C, void* stream);
int sr_norm_act_bwd_nhwc(const float* grad_out, int64_t g_batch_stride, int g_pix_stride, const float* x,
                         int64_t x_batch_stride, int x_pix_stride, const float* mean, const float* var, float eps,
                         const float* gamma, const float* beta, float act_code, int per_image, int train_stats,
                         float* d_in, int64_t d_batch_stride, int d_pix_stride, float* d_gamma, float* d_beta, int B,
                         int HW, int C, void* workspace, size_t workspace_bytes, void* stream);
int sr_rowsum_nhwc(const float* x, int64_t x_batch_stride, int x_pix_stride, const float* g, int64_t g_batch_stride,
                   int g_pix_stride, int B, int HW, int C, float scale, float* out, void* workspace,
                   size_t workspace_bytes, void* stream);
size_t sr_maxblurpool_bwd_workspace_bytes(int B, int H, int W, int C);
int sr_maxblurpool_bwd_nhwc(const float* grad_out, int64_t g_batch_stride, int g_pix_stride, const float* x,
                            int64_t x_batch_stride, int x_pix_stride, float* grad_in, int64_t d_batch_stride,
                            int d_pix_stride, int B, int H, int W, int C, void* workspace, size_t workspace_bytes,
                            void* stream);
int sr_replicate_pad_nhwc_fwd(const float* x, int64_t x_batch_stride, int x_pix_stride, float* y, int B, int H, int W,
                              int C, int pad, void* stream);
int sr_replicate_pad_nhwc_bwd(const float* grad_padded, float* grad_in, int B, int H, int W, int C, int pad, void* stream);
int sr_im2col7x7s2_nhwc(const float* image, int64_t batch_stride, int64_t chan_stride, int64_t row_stride,
                        int64_t col_stride, float* col, int B, int H, int W, int Kp, void* stream);
size_t sr_dwconv3x3_bwd_workspace_bytes(int B, int Ho, int Wo, int C);
int sr_dwconv3x3_bwd_nhwc(const float* grad_out, int64_t g_batch_stride, int g_pix_stride, const float* x,
                          int64_t x_batch_stride, int x_pix_stride, const float* weight, float* d_in, float* d_weight,
                          int B, int H, int W, int C, int stride, int pad_top, int pad_left, int Ho, int Wo,
                          void* workspace, size_t workspace_bytes, void* stream);
int sr_scale_bwd_nhwc(const float* grad_out, int64_t g_batch_stride, int g_pix_stride, const float* gate,
                      const float* d_pool, float pool_scale, float* d_in, int B, int HW, int C, void* stream);
int sr_small_linear_fwd(const float* x, const float* W, const float* bias, float* pre, float* y, int B, int K, int N,
                        float act_code, void* stream);
int sr_small_linear_bwd(const float* dy, const float* pre, const float* x, const float* W, float* dx, float* dW, float* db,
                        int B, int K, int N, float act_code, void* stream);
int sr_act_in_bwd(const float* grad, const float* pre, float* grad_pre, int64_t n, float act_code, void* stream);
/* out = act(a + b) on dense arrays (b null: act(a)); pre (optional) = a + b */
int sr_add_act_fwd(const float* a, const float* b, float* pre, float* out, int64_t n, float act_code, void* stream);
size_t sr_conv_wgrad_padded_workspace_bytes(int B, int Ho, int Wo, int Cin, int Cout, int ksize);
int sr_conv_wgrad_padded_nhwc(const float* in, int64_t in_batch_stride, int in_pix_stride, const float* grad_out,
                              int64_t g_batch_stride, int g_pix_stride, float* d_weight, int B, int H, int W, int Cin,
                              int Cout, int ksize, int stride, int pad_top, int pad_left, int Ho, int Wo, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ---- 16-bit MFMA convolutions of the autocast training path (csrc/sr_conv16.hip; opt-in: SR_AUTOCAST_MFMA16) ----------
 * The reference trains under 16-bit autocast (options.py:100-101 `precision: 16`, train.py:132): its convolutions multiply
 * 16-bit operands.  sr_conv16_nhwc_fwd is that convolution as an implicit GEMM on v_mfma_f32_32x32x16_{f16,bf16}:
 *     out = round_to(out_dtype, act(sum + bias + residual))
 * 3x3 with stride 1 or 2 and zero padding 1 (output (h + 2 - 3) / stride + 1), or 1x1 with stride 1, on channels-last
 * views (strides in ELEMENTS; arbitrary batch / pixel strides, so channel slices of wider buffers work).  It serves the
 * forward pass and, on the flipped and transposed weight (sr_conv_flip_transpose_weights), the data gradient.
 * Numeric contract: input and residual are fp16 (io_dtype = 1) or bf16 (io_dtype = 2); the weight is rounded ONCE to the same
 * type by sr_conv16_pack_weights (round to nearest even, exactly tensor.to(dtype); an fp16 overflow becomes inf, as under
 * torch autocast); products of two 16-bit values are exact and are summed in fp32 on the matrix pipe, taps and channels in a
 * fixed order per output element (no atomics, no K split: two runs give the same bits); bias (fp32), residual and the
 * activation (`leaky_slope` >= 0: LeakyReLU, SR_ACT_NONE: identity; SR_ACT_SILU is SR_ERR_UNSUPPORTED) are applied in fp32;
 * ONE rounding to nearest even on the way out, to out_dtype = io_dtype, or none with out_dtype = 0 (fp32 output: the heads
 * that feed fp32 losses).  Subnormals (from the CDNA ISA text, NOT measured here): the fp32 C input and D output of
 * an MFMA never flush; its A / B operands follow the wave's MODE denormal controls as VALU operations do, and the compiler's
 * default kernel mode keeps subnormals for fp16 as for fp32, so 16-bit subnormal operands enter the sum as the values they
 * encode (a build with -fgpu-flush-denormals-to-zero may flush the operands, never the accumulator); the fp32 epilogue runs
 * in the same default mode, and the output rounding produces 16-bit subnormals where the value calls for one.
 * Requirements (SR_ERR_UNSUPPORTED otherwise, nothing is launched): Cin % 8 == 0 and Cout % 8 == 0 (eight input channels
 * are one 16-byte access; the output is written in whole 4-channel quads, there is no scalar tail), every batch and pixel
 * stride a multiple of 8 elements, pixel strides >= the channel count, 16-byte aligned `in`, `packed_w`, `residual`, `out`.
 * Cin that is no multiple of the 16-channel MFMA step (8, 24, 40, ...) and Cout that is no multiple of the 32-channel tile
 * (8, 40, 160) are zero-filled inside the kernel; nothing is read past a row.  SR_ERR_INVALID_ARGUMENT: a NULL in / packed_w
 * / out, io_dtype outside {1, 2}, out_dtype outside {0, io_dtype}, k outside {1, 3}, stride outside {1, 2} or 2 with k = 1.
 * sr_conv16_supported: the shape test alone (pure host function; pointers and strides are checked at launch).
 * sr_conv16_prefers: 1 where the kernel measured faster than the path the same 16-bit tensors took before it
 * (profiles/r07_conv16.txt) -- what SR_AUTOCAST_MFMA16=1 routes by.  sr_conv16_packed_weight_bytes: size of `packed`
 * (>= 2 Cout Cin k k, a multiple of 16; `packed` must be 16-byte aligned).  Nothing here allocates or synchronises. */
size_t sr_conv16_packed_weight_bytes(int Cout, int Cin, int k);
int sr_conv16_pack_weights(const float* weight /* [Co][Ci][k][k] fp32 */, int Cout, int Cin, int k, int dtype, void* packed,
                           void* stream);
int sr_conv16_supported(int B, int H, int W, int Cin, int Cout, int k, int stride);
int sr_conv16_prefers(int B, int H, int W, int Cin, int Cout, int k, int stride);
int sr_conv16_nhwc_fwd(const void* in, int64_t in_batch_stride, int in_pix_stride, const void* packed_w, const float* bias,
                       const void* residual, int64_t res_batch_stride, int res_pix_stride, void* out,
                       int64_t out_batch_stride, int out_pix_stride, int B, int H, int W, int Cin, int Cout, int k, int stride,
                       float leaky_slope, int io_dtype, int out_dtype, void* stream);

/* ---- 16-bit-operand weight gradient and elementwise backward of the same path (csrc/sr_conv16_wgrad.hip; opt-in:
 * SR_AUTOCAST_MFMA16_WGRAD) --------------------------------------------------------------------------------------------
 * sr_conv16_wgrad_nhwc: d_weight[co][ci][ky][kx] = sum over b, y, x of grad_out[b,y,x,co] * in[b, s y + ky - p, s x + kx - p, ci]
 * for 3x3 at stride 1 or 2 with zero padding 1 and 1x1 at stride 1 (the forms sr_conv16_supported accepts), on
 * v_mfma_f32_32x32x16_{f16,bf16} with M = co, N = ci, K = output pixels.  `in` [B,H,W,Cin] and `grad_out` [B,Ho,Wo,Cout] are
 * fp16 (io_dtype = 1) or bf16 (io_dtype = 2) channels-last views (strides in ELEMENTS; arbitrary batch / pixel strides, so
 * channel slices of wider buffers work); d_weight is fp32, dense [Cout][Cin][k][k], WRITTEN, not accumulated.
 * Numeric contract: products of two 16-bit values are exact and are summed in fp32 on the matrix pipe, in an order that is a
 * function of the shape only -- a workgroup adds its (image, output row, 32-pixel segment) items in index order into one
 * partial slab, a second kernel adds the slabs of a (co, ci) block in index order; no atomics, two runs give the same bits.
 * The output is NOT rounded.  Subnormal operands: as for sr_conv16_nhwc_fwd.  Padding taps, pixels past Wo and channels past
 * Cin / Cout inside a 64-channel block enter the sum as exact zeros on BOTH sides: no result depends on memory outside the
 * operands or on the previous contents of `d_weight` / `workspace`.
 * Workspace: sr_conv16_wgrad_workspace_bytes = blocks x slabs x k k x 64 x 64 x 4 bytes with
 *     blocks = ceil(Cout / 64) ceil(Cin / 64),   slabs (per block) = min(ceil(512 / blocks), B Ho ceil(Wo / 32)),
 * a multiple of 16; 0 for a shape sr_conv16_wgrad_supported refuses.
 * Requirements (SR_ERR_UNSUPPORTED otherwise, nothing is launched): Cin % 8 == 0 and Cout % 8 == 0, every batch and pixel
 * stride a multiple of 8 elements, pixel strides >= the channel count, 16-byte aligned `in` and `grad_out`, a 16-byte aligned
 * `workspace` of at least sr_conv16_wgrad_workspace_bytes bytes.  SR_ERR_INVALID_ARGUMENT: a NULL in / grad_out / d_weight /
 * workspace, io_dtype outside {1, 2}, k outside {1, 3}, stride outside {1, 2} or 2 with k = 1, B <= 0.  Index arithmetic across
 * images is 64-bit.
 * sr_conv16_wgrad_supported: the shape test alone (sr_conv16_supported's forms and channel rules; 0 for B <= 0); pure host
 * function, like sr_conv16_wgrad_workspace_bytes.  sr_conv16_wgrad_prefers: the routing rule of SR_AUTOCAST_MFMA16_WGRAD=1 --
 * 1 for the shape classes where this path measured faster than the fp32 one around its casts (profiles/r08_conv16_wgrad.txt:
 * every conv-stack class measured, 0.25 - 0.86 x the time), 0 for every class nobody measured.
 * sr_act_bwd_bias16_nhwc: sr_act_bwd_bias_nhwc without casts, one pass over a dense [pixels, C] gradient, C % 8 == 0, 16-byte
 * accesses: `grad` is fp32 (grad_dtype = 0: heads that feed fp32 losses) or the layer's 16-bit type (grad_dtype = io_dtype),
 * `out_saved` 16-bit or NULL (no activation), grad_pre (16-bit; may be NULL without an activation: then only d_bias is
 * computed) = round_to(io_dtype, grad * LeakyReLU'(out_saved)), the product in fp32 with ONE rounding to nearest even;
 * d_bias (fp32, or NULL) = the sum over pixels of the UNROUNDED fp32 products, per-block partial sums in `workspace`
 * (sr_act_bwd_bias16_workspace_bytes; SR_ERR_WORKSPACE_TOO_SMALL) added in block order: deterministic.  SR_ERR_UNSUPPORTED:
 * C % 8 != 0 or a pointer that is not 16-byte aligned; SR_ERR_INVALID_ARGUMENT: io_dtype outside {1, 2}, grad_dtype outside
 * {0, io_dtype}, a NULL grad, out_saved without grad_pre, a negative slope. */
int sr_conv16_wgrad_supported(int B, int H, int W, int Cin, int Cout, int k, int stride);
int sr_conv16_wgrad_prefers(int B, int H, int W, int Cin, int Cout, int k, int stride);
size_t sr_conv16_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout, int k, int stride);
int sr_conv16_wgrad_nhwc(const void* in, int64_t in_batch_stride, int in_pix_stride, const void* grad_out,
                         int64_t g_batch_stride, int g_pix_stride, float* d_weight, int B, int H, int W, int Cin, int Cout,
                         int k, int stride, int io_dtype, void* workspace, size_t workspace_bytes, void* stream);
size_t sr_act_bwd_bias16_workspace_bytes(int64_t pixels, int C);
int sr_act_bwd_bias16_nhwc(const void* grad, int grad_dtype, const void* out_saved, void* grad_pre, float* d_bias,
                           int64_t pixels, int C, float leaky_slope, int io_dtype, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ------------------------------------------------------------------ optimiser ----------
 *
 * sr_adamw_step: one AdamW step (decoupled weight decay) on every parameter tensor of a model, two launches whatever the
 * number of tensors.  The rule is torch/optim/adam.py, _single_tensor_adam, non-capturable branch with
 * decoupled_weight_decay=True, per element in fp32 with the roundings of torch's CPU kernels: IEEE sqrt and division,
 * every operation rounded separately except the two marked fma, which ATen's lerp and addcmul fuse as well:
 *     g  = grad / grad_scale                         only when grad_scale is given
 *     p  = p * float(1 - lr * wd)
 *     m  = lerp(m, g, w = float(1 - beta1))          w < 0.5 ? fma(w, g - m, m) : fma(w - 1, g - m, g)
 *     v  = v * float(beta2);  v = fma(float(1 - beta2) * g, g, v)
 *     p  = p + (-float(lr / bc1) * m) / (sqrt(v) / float(sqrt(bc2)) + float(eps))
 *     bc1 = 1 - beta1^step, bc2 = 1 - beta2^step     in double, step = the TENSOR's own count after this step
 * Scalars in float(...) are computed in double and rounded once, as torch rounds a Python float.
 *
 * Tables, all on the device, T = num_tensors entries each: p_ptrs / g_ptrs / m_ptrs / v_ptrs 64-bit addresses of fp32
 * arrays of numel[t] elements (4-byte aligned at least; m and v must not overlap anything else); g_ptrs[t] = 0 says the
 * tensor has no gradient this step: it is not touched and its step count does not advance.  chunk_start int32 [T + 1] =
 * prefix sums of ceil(numel[t] / SR_ADAMW_CHUNK), num_chunks = chunk_start[T]; group int32 [T] = index into the group
 * table; steps fp32 [T] the per-tensor step counts (whole numbers), scalars fp32 [T][2] scratch the call owns.  The
 * kernels trust the tables.  groups_host: num_groups records of SR_ADAMW_GROUP_DOUBLES doubles (lr, beta1, beta2, eps,
 * weight_decay) in HOST memory, read before the call returns and handed to the kernels by value.
 *
 * Launch 1, one thread per tensor with a gradient: steps[t] += 1, scalars[t] = (float(lr / bc1), float(sqrt(bc2))).
 * Launch 2, one workgroup per chunk: finds its tensor by bisecting chunk_start, updates SR_ADAMW_CHUNK consecutive
 * elements (fewer in a tensor's last chunk).  A tensor whose four arrays are all 16-byte aligned moves 16 bytes per lane
 * and access and the last numel % 4 elements as single floats; any other tensor (a slice of a larger buffer, a gradient
 * bucket view) moves single floats throughout.  Same values either way.  The step reads p, g, m, v and writes p, m, v:
 * 28 bytes per element.  Gradients are only read: the unscaled gradient is NOT written back.
 *
 * grad_scale / found_inf: device fp32 scalars or NULL (torch.amp.GradScaler's).  With *found_inf != 0 both launches
 * leave at once: no parameter, moment or step count changes.
 * SR_ERR_INVALID_ARGUMENT: a NULL table, a misaligned table, num_tensors < 1, num_chunks < 0 (0: only launch 1 runs),
 * num_groups < 1, a group with a negative or NaN lr / eps / weight_decay or a beta outside [0, 1).  SR_ERR_UNSUPPORTED:
 * num_tensors above SR_ADAMW_MAX_TENSORS, num_groups above SR_ADAMW_MAX_GROUPS.  No call allocates or synchronises with
 * the host; results are elementwise and equal bit for bit on every run. */
#define SR_ADAMW_CHUNK 4096
#define SR_ADAMW_MAX_GROUPS 16
#define SR_ADAMW_MAX_TENSORS (1 << 20)
#define SR_ADAMW_GROUP_DOUBLES 5
int sr_adamw_step(const void* p_ptrs, const void* g_ptrs, const void* m_ptrs, const void* v_ptrs, const int64_t* numel,
                  const int32_t* chunk_start, const int32_t* group, float* steps, float* scalars, int num_tensors,
                  int num_chunks, const double* groups_host, int num_groups, const float* grad_scale,
                  const float* found_inf, void* stream);

/* sr_adamw_step_clipped: sr_adamw_step with one more optional device scalar, grad_coef (fp32, 4-byte aligned, or NULL):
 * after `g = grad / grad_scale` the kernel computes `g = g * *grad_coef`, rounded separately, in registers.  One kernel
 * body serves both entry points: sr_adamw_step forwards with grad_coef = NULL, and a coefficient of exactly 1.0f changes
 * no bit of any result.
 *
 * sr_grad_stats: gradient norms, the non-finite flag, torch's clip coefficient and (optionally) the loss scaler's update,
 * in two launches over the tables of sr_adamw_step (g_ptrs, numel, chunk_start, num_tensors, num_chunks).  Gradients are
 * only read.
 *   Launch 1, one 256-lane workgroup per chunk: every element is converted to DOUBLE, squared and added; a fixed-order
 *   wave and LDS reduction writes one double per chunk into the workspace (0 for a tensor whose address is 0).  16-byte
 *   loads for 16-byte aligned tensors, single floats for the numel % 4 tail and for every other tensor.
 *   Launch 2, one workgroup: per tensor the sum of its partials in chunk order, then the sum over the tensors in index
 *   order; no atomics, so two runs give the same bytes.  With s = *grad_scale (or *scaler_scale, or 1 without either)
 *   it writes, all fp32:
 *     norms[t]                        sqrt(sum_t) / s, computed in double and rounded once: the norm of the UNSCALED gradient
 *     stats[SR_GRAD_STATS_NORM]       the same over all tensors
 *     stats[SR_GRAD_STATS_FOUND_INF]  1.0 when the total sum is not finite, else 0.0
 *     stats[SR_GRAD_STATS_COEF]       max_norm > 0: q = max_norm / (norm + 1e-6f) in fp32, each operation rounded, then
 *                                     q > 1 ? 1 : q (torch.nn.utils.clip_grad_norm_; a NaN stays); otherwise 1.0
 *     stats[SR_GRAD_STATS_SCALE]      s, the scale of THIS step: what sr_adamw_step_clipped divides by when the scaler's
 *                                     own slot is updated in the same launch
 *   The flag is equivalent to "some element is not finite": the square of a finite fp32 value is below 2^256 and a sum
 *   of fewer than 2^31 of them is finite in double, while inf and NaN carry through the square and every addition of
 *   non-negative terms.  Double also keeps gradients of 1e30 or 1e-30, whose squares leave the fp32 range, and makes the
 *   sum independent of the order to 2^-26 relatively, far below fp32 resolution.
 *   scaler_scale (fp32) / scaler_tracker (int32), both or neither, and not together with grad_scale: torch's
 *   _amp_update_scale_ at the end of launch 2.  Flag set: scale = float(scale * backoff_factor), tracker = 0.  Otherwise
 *   tracker += 1, and when it reaches growth_interval: scale = float(scale * growth_factor) if that is finite, tracker = 0.
 * workspace: sr_grad_stats_workspace_bytes(num_chunks, num_tensors) bytes, 8-byte aligned; every byte a launch reads was
 * written by launch 1 of the same call.
 *
 * sr_grad_scale_inplace: g[i] = g[i] * *coef for every element of every tensor with a gradient, one launch over the same
 * chunk table (the in-place half of torch's clip_grad_norm_, which always multiplies).
 *
 * SR_ERR_INVALID_ARGUMENT: a NULL or misaligned table, output or scalar, num_tensors < 1, num_chunks < 0, a NaN max_norm,
 * one scaler pointer without the other or together with grad_scale, a factor that is not positive, growth_interval < 1.
 * SR_ERR_UNSUPPORTED: num_tensors above SR_ADAMW_MAX_TENSORS.  SR_ERR_WORKSPACE_TOO_SMALL.  No call allocates or
 * synchronises with the host. */
#define SR_GRAD_STATS_NORM 0
#define SR_GRAD_STATS_FOUND_INF 1
#define SR_GRAD_STATS_COEF 2
#define SR_GRAD_STATS_SCALE 3
#define SR_GRAD_STATS_SLOTS 4
int sr_adamw_step_clipped(const void* p_ptrs, const void* g_ptrs, const void* m_ptrs, const void* v_ptrs,
                          const int64_t* numel, const int32_t* chunk_start, const int32_t* group, float* steps,
                          float* scalars, int num_tensors, int num_chunks, const double* groups_host, int num_groups,
                          const float* grad_scale, const float* found_inf, const float* grad_coef, void* stream);
size_t sr_grad_stats_workspace_bytes(int num_chunks, int num_tensors);
int sr_grad_stats(const void* g_ptrs, const int64_t* numel, const int32_t* chunk_start, int num_tensors, int num_chunks,
                  const float* grad_scale, float max_norm, float* norms, float* stats, float* scaler_scale,
                  int32_t* scaler_tracker, double growth_factor, double backoff_factor, int growth_interval,
                  void* workspace, size_t workspace_bytes, void* stream);
int sr_grad_scale_inplace(const void* g_ptrs, const int64_t* numel, const int32_t* chunk_start, int num_tensors,
                          int num_chunks, const float* coef, void* stream);

/* ---- offline and dense tuple generation (sr_tuples.hip; reference data_scripts/generate_test_tuples.py:65-157, 268-382,
 * tools/keyframe_buffer.py:245-381) -----------------------------------------------------------------------------------
 * sr_pose_inverse_f64: inverses[i] = poses[i]^-1 for n row-major 4x4 fp64 matrices, a general inverse by cofactors (no
 * rigid-motion shortcut; a singular matrix gives inf / NaN).
 *
 * sr_tuple_walk_f64: one walk per entry of reference_indices [n_walks] (int32 frame numbers into poses [n_poses,4,4] and
 * their inverses), one wave each.  The walk is primed with its reference frame r and offers, in this order, r+1, r-1,
 * r+2, r-2, ... (both_directions != 0; a direction that has run out still takes its turn) or r-1, r-2, ... (0) to a FIFO
 * of buffer_size poses: a candidate c is admitted when sqrt(t^2 + R^2) of inv(pose c) @ pose b reaches
 * keyframe_pose_distance for every buffered b (R = sqrt(2 (1 - min(3, trace) / 3)), t = |translation|); admitted into a full
 * buffer it pushes the oldest entry out, the primed frame first.  The walk ends when both directions have run out or after a
 * candidate's test has left acceptance_cap admissions behind it.  Then the oldest entry is dropped, the next one becomes
 * the reference pose of the penalties (R - optimal_r)^2 + w (t - optimal_t)^2, w = 5 below optimal_t and 1 from it on,
 * of inv(reference) @ pose b over all entries left, itself included, and the min(n_measurement_frames, entries left - 1)
 * smallest are the sources.  indices [n_walks, 1 + n_measurement_frames] int32: r, then the sources by ascending penalty
 * (ties: older entry first), then -1; counts [n_walks]: the number of sources.  A reference index outside [0, n_poses) gives
 * a row of -1 and count 0.  Every byte of both outputs is written; fp64 throughout; no atomics, no workspace, no
 * synchronisation: the same call gives the same bytes.
 * Poses must be finite with a bottom row of exactly 0 0 0 1 (the kernel reads rows 0..2 only); the caller checks.
 * SR_ERR_UNSUPPORTED: buffer_size > 64 (one slot per lane), n_measurement_frames > 63.  SR_ERR_INVALID_ARGUMENT: negative
 * sizes, buffer_size < 1, n_poses > 2^28, a NULL pointer (poses may be NULL when n_poses == 0), fp64 pointers not 8-byte or
 * int32 pointers not 4-byte aligned. */
int sr_pose_inverse_f64(const double* poses, double* inverses, int n, void* stream);
int sr_tuple_walk_f64(const double* poses, const double* inverses, int n_poses, const int32_t* reference_indices,
                      int n_walks, int both_directions, int buffer_size, int acceptance_cap,
                      double keyframe_pose_distance, double optimal_t, double optimal_r, int n_measurement_frames,
                      int32_t* indices, int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLERECON_HIP_H_ */
