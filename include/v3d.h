/*
 * v3d.h -- C ABI of lib3dvnet_hip.so: MI355X (gfx950) kernels for 3DVNet's plane-sweep
 * cost-volume and volumetric-refinement hot path.
 *
 * The reference (alexrich021/3dvnet) has no FFI layer: the path sits behind PyTorch nn.Module
 * methods whose arithmetic lives in torch / torch_scatter / MinkowskiEngine CUDA kernels.  Each
 * entry point below replaces one such fused region; the reference call sites it replaces are
 * cited per function (paths relative to the reference root).  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (tensor.data_ptr()) unless the name ends in `_host`;
 *     tensors are contiguous; float = IEEE f32; indices int32 unless noted;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     calls only enqueue work on it and never synchronise;
 *   - the library never allocates or frees tensor memory: outputs and scratch are allocated by
 *     the caller, `*_workspace_bytes()` reports scratch sizes.  The only library-owned device
 *     memory is inside weight handles (`v3d_*_pack` / `v3d_*_free`);
 *   - return value: 0 = V3D_OK, negative = error; `v3d_last_error()` returns a thread-local
 *     message.  No C++ exception crosses the boundary.
 *
 * Workspace and output contract (enforced per entry point by tests/test_workspace_contract_gpu.py over the table
 * tests/workspace_cases.py)
 *   - the contents of every workspace, hash table and output buffer on entry are arbitrary: a call reads no byte of them
 *     that it, or an earlier call of the same documented chain, has not written.  Every element an entry point is said to
 *     write is stored, whatever the buffer held;
 *   - a workspace may be handed to any later call, of any entry point and any shape it is large enough for;
 *   - no call writes outside `*_workspace_bytes()` / `v3d_hash_bytes()` bytes of its workspace or outside the documented size
 *     of an output (where a length comes back from the call -- unique keys, compacted points, mesh rows, down-sampled cells --
 *     rows beyond it are unspecified but inside the buffer);
 *   - a status word (v3d_edges_csr_status, v3d_voxelize_status, v3d_hash_status, v3d_cloud_status, *status of
 *     v3d_mesh_render_depth_f32) describes the most recent call on that workspace only: a rejected input leaves nothing behind.
 *   Exceptions, each stated again at its entry point: buffers a call accumulates into are the caller's state (tsdf / weight /
 *   color of v3d_tsdf_integrate_f32, `pool` of v3d_gemm_gather_f32, depth_inout of v3d_decoder_fused_f32); a hash table is an
 *   INPUT of v3d_sparse_neighbors / v3d_sparse_interp_f32 / v3d_decoder_fused_f32; the chains keep what the first call left in
 *   the workspace -- v3d_voxel_keys -> v3d_voxel_decode / v3d_voxelize_status, v3d_mesh_count_f32 -> v3d_mesh_extract_f32,
 *   v3d_cloud_downsample_f32 -> v3d_cloud_status, v3d_edges_csr -> v3d_edges_csr_status, and the channel-last feature copy of
 *   v3d_backproject_variance_f32 for a following call with feat == NULL.
 */
#ifndef V3D_H_
#define V3D_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define V3D_OK 0
#define V3D_ERR_BAD_SHAPE (-1)
#define V3D_ERR_BAD_ARG (-2)
#define V3D_ERR_WORKSPACE_TOO_SMALL (-3)
#define V3D_ERR_HIP (-4)
#define V3D_ERR_UNSUPPORTED (-5)

/* Arithmetic of the matrix-core kernels (every entry point that takes `precision`).  Storage and accumulation are
 * fp32 in both modes; the modes differ in the MFMA operands:
 *   V3D_PRECISION_SPLIT_BF16  each fp32 operand x = hi + lo (hi = RNE_bf16(x), lo = RNE_bf16(x - hi), 16 mantissa bits);
 *                             product = hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 (lo*lo dropped).  Narrower than
 *                             the reference's fp32; passes the 1e-4 relative depth gate of BASELINE.json (the default of
 *                             the Python modules and of bench.py's headline value).
 *   V3D_PRECISION_FP32        exact fp32 products on v_mfma_f32_16x16x4_f32 (bitwise an fmaf chain) -- the reference's
 *                             arithmetic type; about 2x slower on the regulariser. */
#define V3D_PRECISION_SPLIT_BF16 0
#define V3D_PRECISION_FP32 1

/* Developer options: process-wide integers the launch paths read (they replace the environment variables of earlier rounds; a
 * production caller never needs them -- every default is the shipped path).  Names / values:
 *   "psv_kernel"      0 auto (window kernel; reuse kernel for feature stacks >= 2 GB) | 1 reuse kernel | 2 gather kernel
 *   "c12_march"       1 conv1 + conv2 of CostRegNet as one depth march | 0 the two tile kernels (another summation order of conv2)
 *   "stop_after"      layer after which v3d_costreg_depth_* returns (-DV3D_PHASE_TIMING builds)
 *   "gemm_rounds"     1 | 0      gather-GEMM in rounds for small M | the one-step kernel (bit-identical)
 *   "gemm_pipe"       1 | 0      sparse convolutions on the loader / matrix pipeline kernel | the rounds kernel (bit-identical)
 *   "psv_walk"        0 | N      plane chunks (of 8 planes) a wave of the window warp kernel walks: chosen from the shape | N (bit-identical)
 *   "render_coop"     N          v3d_mesh_render_depth_f32: bounding boxes of more than N pixels are rasterised by the whole wave,
 *                                smaller ones by the triangle's own thread (default 64; 0 = every box; bit-identical)
 *   "psv_skip"        1 | 0      the window warp kernel skips an (edge, 8 planes, 8 pixels) pass whose samples all fall beside the
 *                                source image (they add exactly zero) | never skips (bit-identical)
 * Unknown names, gemm_rounds / gemm_pipe / psv_skip / wgrad_compact values other than 0 and 1, and a negative psv_walk / render_coop -> V3D_ERR_BAD_ARG.
 * ("psv_walk", "render_coop", "psv_skip" and "wgrad_compact" are additive within ABI version 9: new option names, no changed signature; v3d_version() is not
 * bumped.) */
int v3d_set_option(const char* name, int value);
int v3d_get_option(const char* name, int* value);

/* ABI version (bumped on any signature change) and last error text of the calling thread. */
int v3d_version(void);
const char* v3d_last_error(void);

/* Diagnostics (no reference counterpart): when enabled, every kernel launched by the library is
 * bracketed by hipEvents on its stream; v3d_timing_collect synchronises them, sums the elapsed time
 * per kernel name and clears the log.  names: max_entries x name_stride chars (HOST memory). */
int v3d_timing_enable(int on);
int v3d_timing_collect(int max_entries, char* names_host, int name_stride, float* total_ms_host,
                       int* launches_host);

/* ------------------------------------------------------------------------------------------
 * Row A7 bookkeeping: edge list -> per-reference CSR on the device, no host round trip.
 * Replaces mvsnet.py:179 (ref_idx, gather_idx = torch.unique(ref_src_edges[0], return_inverse=True), whose output length
 * the host must read back) and the grouping scatter(.., gather_idx) implies at mvsnet.py:214-215.
 *
 *   edges     [2, n_edges] int64 (row 0 = reference image, row 1 = source image), any order
 *   n_ref     the number of distinct reference images, known to the caller (the batch holds that many depth maps)
 *   ref_img   [n_ref]      out: ascending distinct values of edges[0] (= torch.unique's order)
 *   edge_ofs  [n_ref+1]    out: first edge of every reference in edge_src
 *   edge_src  [n_edges]    out: edges[1] grouped per reference, original edge order inside a group
 *   workspace >= v3d_edges_csr_workspace_bytes(n_img, n_ref)
 * If n_ref is not the number of distinct references, or an index is outside [0, n_img), the kernel writes an empty CSR
 * (all n_ref + 1 offsets 0 AND all n_ref entries of ref_img 0: the consumers read ref_img[r] and that image's camera block
 * even for a reference without edges, so both tables keep them inside their buffers; the result is a zero variance
 * volume) and sets the workspace's error word; v3d_edges_csr_status copies it to the host (synchronises) ->
 * V3D_ERR_BAD_SHAPE.  Nothing downstream reads that word: callers check it once per edge list (Python: EdgeCsr.check(),
 * MVSNet.check_edges(); CostVolumeGraph checks at capture and on update(ref_src_edges=)).
 * ------------------------------------------------------------------------------------------ */
size_t v3d_edges_csr_workspace_bytes(int n_img, int n_ref);
int v3d_edges_csr(const int64_t* edges, int n_edges, int n_img, int n_ref, int32_t* ref_img, int32_t* edge_ofs,
                  int32_t* edge_src, void* workspace, size_t workspace_bytes, void* stream);
int v3d_edges_csr_status(const void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Rows A1-A4: plane-sweep warp + cross-view variance, one fused kernel.
 * Replaces mv3d/utils.py:86-108 (batched_build_plane_sweep_volume_tensor),
 * mv3d/subnetworks/mvsnet.py:192-206 (projection, |z|+1e-8, normalisation),
 * mvsnet.py:209-211 (F.grid_sample bilinear/zeros/align_corners=True) and
 * mvsnet.py:214-216 (two torch_scatter means -> variance).
 *
 *   feat      [n_img, C, Hf, Wf]  quarter-resolution features (C in {16, 32})
 *   K, R, t   [n_img,3,3], [n_img,3,3], [n_img,3]   intrinsics at image size, world->camera
 *   ref_img   [n_ref]      image index of each reference view (ascending = torch.unique order)
 *   edge_ofs  [n_ref+1]    CSR offsets into edge_src (edges grouped per reference, original order)
 *   edge_src  [n_edges]    source image index per edge
 *   H, W      image size the intrinsics refer to; h, w = plane grid; D planes at
 *             depth_start + i*depth_interval (float32 values of numpy.linspace, utils.py:94)
 *   var       [n_ref, C, D, h, w] out
 *   workspace >= v3d_psv_workspace_bytes(n_img, C, Hf, Wf) bytes, 256-byte aligned
 * ------------------------------------------------------------------------------------------ */
size_t v3d_psv_workspace_bytes(int n_img, int C, int Hf, int Wf);
/* Diagnostic (no reference counterpart): the number of consecutive 8-plane chunks a wave of the window warp kernel walks for a
 * launch of n_ref views, D planes and an h x w plane grid -- a function of the shape alone, or the developer option "psv_walk"
 * when that is set; at most the number of chunks.  Additive within ABI version 9. */
int v3d_psv_walk_chunks(int n_ref, int D, int h, int w);
int v3d_psv_variance_f32(const float* feat, const float* K, const float* R, const float* t,
                         const int32_t* ref_img, const int32_t* edge_ofs, const int32_t* edge_src,
                         int n_img, int n_ref, int n_edges, int C, int Hf, int Wf, int H, int W,
                         double depth_start, double depth_interval, int D, int h, int w,
                         float* var, void* workspace, size_t workspace_bytes, void* stream);

/* Diagnostic twin of the projection inside v3d_psv_variance_* (rows A1-A2 + grid_sample's un-normalisation): the sample
 * position (ix, iy), in feature-map pixels, of every (edge, plane, pixel) -- computed by the same device functions the warp
 * kernels use, so tests can compare the coordinates with the reference's bit for bit.
 *   pos   [n_edges, D*h*w, 2] out;  world [n_ref, 3, D*h*w] out, optional (NULL to skip): the plane-sweep points (row A1)
 *   workspace >= n_img * 36 floats */
int v3d_psv_sample_positions_f32(const float* K, const float* R, const float* t, const int32_t* ref_img,
                                 const int32_t* edge_ofs, const int32_t* edge_src, int n_img, int n_ref, int n_edges,
                                 int Hf, int Wf, int H, int W, double depth_start, double depth_interval, int D, int h,
                                 int w, float* pos, float* world, void* workspace, size_t workspace_bytes, void* stream);

/* Same computation, but `var_split` receives the volume in the regulariser's private input format (no
 * reference counterpart; it only exists to keep the 1.2 GB volume from being re-formatted by the next kernel):
 * every fp32 value x stored as bf16 hi = RNE(x) and bf16 lo = RNE(x - hi), channel-last in 16-byte slots of
 * 8 channels, [n_ref][4 channel groups][hi, lo][D][h][w][8].  n_ref*C*D*h*w*4 bytes like `var`; C must be 32.
 * hi + lo reproduces what conv0's own on-the-fly split of `var` produces, bit for bit. */
int v3d_psv_variance_split(const float* feat, const float* K, const float* R, const float* t,
                         const int32_t* ref_img, const int32_t* edge_ofs, const int32_t* edge_src,
                         int n_img, int n_ref, int n_edges, int C, int Hf, int Wf, int H, int W,
                         double depth_start, double depth_interval, int D, int h, int w,
                         void* var_split, void* workspace, size_t workspace_bytes, void* stream);

/* The same volume as fp32 in the channel-last layout of the exact-fp32 chain's conv0 (V3D_PRECISION_FP32 through
 * v3d_costreg_depth_cl8): [n_ref][4 channel groups][2 halves][D][h][w] 16-byte slots of 4 floats -- half 0 = channels 0..3
 * of the group, half 1 = channels 4..7.  The numbers are those of v3d_psv_variance_f32, bit for bit; C must be 32. */
int v3d_psv_variance_cl8(const float* feat, const float* K, const float* R, const float* t,
                         const int32_t* ref_img, const int32_t* edge_ofs, const int32_t* edge_src,
                         int n_img, int n_ref, int n_edges, int C, int Hf, int Wf, int H, int W,
                         double depth_start, double depth_interval, int D, int h, int w,
                         float* var_cl8, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Rows A5-A6: CostRegNet (dense 3D-conv U-Net, BatchNorm folded) + soft-argmin depth.
 * Replaces mvsnet.py:133-163 (CostRegNet.forward) and mvsnet.py:219-227.
 *
 * v3d_costreg_pack takes HOST pointers to the reference state_dict tensors
 * (mvsnet.py:136-152; conv{0..6}.conv.weight [Co,Ci,3,3,3], conv{7,8,9}.deconv.weight
 * [Ci,Co,3,3,3], *.bn.{weight,bias,running_mean,running_var}, prob.weight [1,base,3,3,3],
 * prob.bias [1]), folds eval-mode BatchNorm (eps) into the convolutions, re-orders the weights
 * into MFMA fragment order and uploads them.  Order of the 10 conv/deconv layers in the arrays:
 * conv0..conv9.  Built: (in_channels, base_channels) = (32, 8) -- mv3d/config.py:42 -- and (16, 8), the
 * reference's signature default feat_dim (lightningmodel.py:18); a 16-channel net takes its variance
 * volume through v3d_costreg_depth_f32 only (the split / channel-last hand-off formats are defined
 * for 32 channels).
 * ------------------------------------------------------------------------------------------ */
typedef struct v3d_costreg_weights v3d_costreg_weights;

int v3d_costreg_pack(const float* const* conv_weight_host, const float* const* bn_weight_host,
                     const float* const* bn_bias_host, const float* const* bn_mean_host,
                     const float* const* bn_var_host, const float* prob_weight_host,
                     const float* prob_bias_host, int in_channels, int base_channels, float bn_eps,
                     v3d_costreg_weights** out_handle);
void v3d_costreg_free(v3d_costreg_weights* handle);

/*   var        [n_ref, Cin, D, h, w] in   (D, h, w divisible by 8)
 *   depth_vals [D]  depth hypothesis values (torch.linspace(depth_start, depth_end, D), :223)
 *   depth      [n_ref, h, w] out
 *   reg        [n_ref, D, h, w] out, optional (NULL to skip): the regularised volume x_reg
 *   workspace  >= v3d_costreg_workspace_bytes(...) */
size_t v3d_costreg_workspace_bytes(const v3d_costreg_weights* handle, int n_ref, int D, int h, int w);
int v3d_costreg_depth_f32(const v3d_costreg_weights* handle, const float* var,
                          const float* depth_vals, int n_ref, int D, int h, int w, float* depth,
                          float* reg, int precision, void* workspace, size_t workspace_bytes, void* stream);
/* As above with the variance volume in the split format written by v3d_psv_variance_split (the split format IS the
 * V3D_PRECISION_SPLIT_BF16 operand encoding, so this entry point has no precision argument). */
int v3d_costreg_depth_split(const v3d_costreg_weights* handle, const void* var_split,
                          const float* depth_vals, int n_ref, int D, int h, int w, float* depth,
                          float* reg, void* workspace, size_t workspace_bytes, void* stream);
/* As v3d_costreg_depth_f32 with V3D_PRECISION_FP32 (exact fp32 products) and the volume in the fp32 channel-last layout
 * of v3d_psv_variance_cl8: conv0 then runs as a depth march that streams the volume with LDS-DMA (csrc/conv0z.hip). */
int v3d_costreg_depth_cl8(const v3d_costreg_weights* handle, const void* var_cl8,
                          const float* depth_vals, int n_ref, int D, int h, int w, float* depth,
                          float* reg, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Photometric confidence of a plane-sweep depth (additive within ABI version 9; csrc/confidence.hip).
 * Replaces mv3d/utils.py:111-145 (get_propability_map): the probability mass of the two depth planes that bracket a
 * pixel's depth on the grid depth_start + i * depth_interval, i in [0, D).
 *
 * Plane indices -- all fp32, every operation rounded on its own, depth_start and depth_interval rounded to fp32 first
 * (as torch rounds a Python scalar that meets an fp32 tensor):
 *     d = fl(fl(depth - depth_start) / depth_interval)        one subtract, one correctly rounded divide
 *     l = clamp(floor(d), 0, D - 1),  r = clamp(ceil(d), 0, D - 1)
 *   l == r rule: when the depth lies exactly on a plane (d is an integer), or below the first / above the last plane (both
 *     indices clamp to the same end), the SAME value is added twice; the result is 2 p[l] and can reach 2.0.  This is the
 *     reference's behaviour and is kept.  (The fp32 coordinate of a plane's own depth is not always that plane's integer:
 *     of torch.linspace(0.5, 5.25, 96) 68 planes land on it, 9 above, 19 below; each follows the rule above as it falls.)
 *   NaN rule: a d that is NaN or +-infinite (a NaN or infinite depth) is never converted to an integer: l = r = 0, the
 *     result is 2 p[0].  (x86's float -> int64 conversion, which the reference runs into, gives the same index.)  A finite d
 *     of any size clamps to 0 or D - 1.
 * Values:
 *   v3d_probability_map_f32    cv [n, D, h, w] already holds probabilities: prob = fl(cv[l] + cv[r]).
 *   v3d_confidence_logits_f32  x_reg [n, D, h, w] holds the regulariser's logits; p = softmax(-x_reg) over D is never
 *     written: one walk over D keeps the running maximum m of -x and den = sum_d expf(-x_d - m), in the order of operations
 *     of the soft-argmin (rescaling den by expf(m_old - m_new) whenever the maximum moves), then
 *     prob = fl(fl(expf(-x[l] - m) / den) + fl(expf(-x[r] - m) / den)): two correctly rounded divides, then one add --
 *     softmax, gather, add, as the reference orders them.  depth_map [n, h, w] is the caller's.
 *   v3d_costreg_depth_prob     the chain of v3d_costreg_depth_f32 / _split / _cl8 with the input layout and the precision
 *     as arguments.  prob == NULL: exactly those entry points (same kernels, same launches).  prob [n_ref, h, w] given: the
 *     last kernel is the soft-argmin that also writes the confidence of its OWN depth: the depth has the bits of the other
 *     entry points, prob the bits v3d_confidence_logits_f32 gives for that x_reg and that depth.  depth_start /
 *     depth_interval describe the grid depth_vals was built from; they are used for the plane indices only.
 * Every argument is validated on the host before any launch: null pointers and a depth_start / depth_interval that is not
 * finite as fp32, or a zero interval -> V3D_ERR_BAD_ARG; n, D, h, w <= 0, D >= 2^24 (and for the regulariser D, h, w not
 * multiples of 8) -> V3D_ERR_BAD_SHAPE.  No workspace besides the regulariser's; repeated launches are bit-identical.
 * ------------------------------------------------------------------------------------------ */
#define V3D_LAYOUT_REFERENCE 0 /* fp32 [n_ref, Cin, D, h, w]            (v3d_costreg_depth_f32)   */
#define V3D_LAYOUT_SPLIT 1     /* v3d_psv_variance_split's hand-off     (v3d_costreg_depth_split) */
#define V3D_LAYOUT_CL8 2       /* v3d_psv_variance_cl8's fp32 hand-off  (v3d_costreg_depth_cl8)   */
int v3d_costreg_depth_prob(const v3d_costreg_weights* handle, const void* var, int in_layout, int precision,
                           const float* depth_vals, double depth_start, double depth_interval, int n_ref, int D, int h,
                           int w, float* depth, float* reg, float* prob, void* workspace, size_t workspace_bytes,
                           void* stream);
/* The last kernel of that chain alone, on an x_reg [n, D, h, w] the caller holds (any D, h, w): depth [n, h, w] = the
 * soft-argmin; prob NULL: the kernel of v3d_costreg_depth_f32, else the kernel that also writes the confidence. */
int v3d_soft_argmin_f32(const float* x_reg, const float* depth_vals, double depth_start, double depth_interval, int n, int D,
                        int h, int w, float* depth, float* prob, void* stream);
int v3d_confidence_logits_f32(const float* x_reg, const float* depth_map, double depth_start, double depth_interval, int n,
                              int D, int h, int w, float* prob, void* stream);
int v3d_probability_map_f32(const float* cv, const float* depth_map, double depth_start, double depth_interval, int n, int D,
                            int h, int w, float* prob, void* stream);

/* Single dense 3D layer of the regulariser (exposed for per-layer parity tests):
 * layer 0..9 = conv0..conv9 of CostRegNet incl. folded BN + ReLU (+ `skip` added after the ReLU
 * when non-NULL, mvsnet.py:159-161).  in [n, Cin, Di, Hi, Wi] -> out [n, Cout, Do, Ho, Wo].
 * precision: V3D_PRECISION_FP32 = the exact-fp32 kernel of every layer; V3D_PRECISION_SPLIT_BF16 = conv0 on its
 * split-bf16 product kernel (the other layers' split-bf16 kernels use the split activation layout: next entry point). */
int v3d_costreg_layer_f32(const v3d_costreg_weights* handle, int layer, const float* in,
                          const float* skip, int n, int Di, int Hi, int Wi, float* out, int precision,
                          void* stream);

/* The same layers 1..8 (conv1..conv8) on the kernels the fused path uses: split-bf16 matrix cores reading the split
 * channel-last activation layout.  `in`, `skip` (conv7 / conv8, required) and `out` are fp32 [n, C, D, H, W]; the
 * input is re-encoded into `workspace` (>= v3d_costreg_layer_split_workspace_bytes).  Layer 0 already runs its
 * product kernel through v3d_costreg_layer_f32; conv9 only exists fused with the prob conv (v3d_costreg_depth_*). */
size_t v3d_costreg_layer_split_workspace_bytes(int n, int cin, int Di, int Hi, int Wi);
int v3d_costreg_layer_split_f32(const v3d_costreg_weights* handle, int layer, const float* in, const float* skip,
                                int n, int Di, int Hi, int Wi, float* out, void* workspace, size_t workspace_bytes,
                                void* stream);

/* ------------------------------------------------------------------------------------------
 * Rows B1-B2 and C1: back-project depth pixels / depth hypotheses to world points and compute their
 * multi-view variance feature.  Replaces mv3d/utils.py:67-83 (build_img_pts),
 * mv3d/lightningmodel.py:138-169 (construct_feature_rich_pointcloud) and :191-229 (run_pointflow).
 *   depth [n_ref, h, w]; feat [n_img, C, Hf, Wf]; cameras / edge CSR as in v3d_psv_variance_f32;
 *   hypotheses depth + i*offset, i in [-n_half, n_half] (n_half = 0: the depth itself);
 *   pts [n_ref*h*w, 2*n_half+1, 3] out, var [n_ref*h*w, 2*n_half+1, C] out (= pts_hyp / pts_feat of
 *   lightningmodel.py:231-235; for n_half = 0: pts / pts_feat of :171-172).
 *   The call keeps a channel-last copy of `feat` in `workspace`; feat == NULL means "the workspace still holds the copy the
 *   previous call made of the same feature tensor" (a driver that sweeps one scene's features repeatedly skips the copy).
 * ------------------------------------------------------------------------------------------ */
size_t v3d_backproject_workspace_bytes(int n_img, int C, int Hf, int Wf);
int v3d_backproject_variance_f32(const float* depth, const float* feat, const float* K, const float* R,
                                 const float* t, const int32_t* ref_img, const int32_t* edge_ofs,
                                 const int32_t* edge_src, int n_img, int n_ref, int n_edges, int C,
                                 int Hf, int Wf, int H, int W, int h, int w, double offset, int n_half,
                                 float* pts, float* var, void* workspace, size_t workspace_bytes,
                                 void* stream);

/* ------------------------------------------------------------------------------------------
 * Gather-GEMM on the matrix cores (fp32 in/out; operands per `precision`): Y[m,:] = epilogue(sum_s act(X_s[row_s(m), 0:K]) @ W_s + bias).
 * Replaces the dense arithmetic of: PointNet's Linear layers incl. the concat with the pooled voxel
 * feature and torch_scatter max (mv3d/subnetworks/scenemodeling.py:127-144); MinkowskiConvolution /
 * ConvolutionTranspose / 1x1 + MinkowskiGroupNorm + ReLU + residual (scenemodeling.py:16-44,160,181,
 * 186); Conv1d+BN+ReLU of the hypothesis decoder (mv3d/subnetworks/refinement.py:8-13,20-23).
 *
 * v3d_gemm_pack: HOST weight tensor addressed as w[seg*stride_seg + co*stride_co + k*stride_k]
 *   (Linear [N, n_seg*K]: K, n_seg*K, 1;  ME kernel [27, Ci, Co]: Ci*Co, 1, Co;  Conv1d [Co, Ci, 3]:
 *   1, 3*Ci, 3), optional per-output scale (folded BatchNorm), bias, GroupNorm affine.  N <= 128.
 * v3d_gemm_gather_f32: seg_src/seg_idx/seg_ld are HOST arrays of n_seg device pointers / strides;
 *   seg_idx[s] NULL = identity row map, entry -1 = zero row; group_len > 0 selects the conv1d row map
 *   (segment s reads row m + s - n_seg/2 inside each group of group_len rows; seg_idx ignored);
 *   relu_in: ReLU applied to gathered inputs; use_gn: per-row GroupNorm (1 or 16: over 16-channel groups, 8: over 8-channel
 *   groups; eps gn_eps) before the optional residual add and ReLU; pool/pool_idx: scatter-max of the result
 *   into pool[pool_idx[m], :] (pre-filled with -inf); out may be NULL.
 * ------------------------------------------------------------------------------------------ */
typedef struct v3d_gemm_weights v3d_gemm_weights;
int v3d_gemm_pack(const float* w_host, long long stride_seg, long long stride_co, long long stride_k,
                  int n_seg, int N, int K, const float* scale_host, const float* bias_host,
                  const float* gn_w_host, const float* gn_b_host, v3d_gemm_weights** out_handle);
void v3d_gemm_free(v3d_gemm_weights* handle);
int v3d_gemm_gather_f32(const v3d_gemm_weights* handle, int M, const float* const* seg_src_host,
                        const int32_t* const* seg_idx_host, const int* seg_ld_host, int group_len,
                        int relu_in, int use_gn, float gn_eps, const float* residual, int ld_res,
                        int relu_out, float* pool, const int32_t* pool_idx, int ld_pool, float* out,
                        int ld_out, int precision, void* stream);
/* A sparse convolution as one call (MinkowskiConvolution / ConvolutionTranspose + MinkowskiGroupNorm + residual + ReLU,
 * scenemodeling.py:16-44,160,181): v3d_gemm_gather_f32 with every segment reading `src` [*, ld_src] through column k of the
 * neighbour table `nbr` ([n_seg, nbr_stride] int32 from v3d_sparse_neighbors, -1 = absent voxel).  Same kernels, same bits;
 * the caller passes 4 pointers instead of three host arrays of n_seg entries. */
int v3d_sparse_conv_f32(const v3d_gemm_weights* handle, int M, const float* src, int ld_src, const int32_t* nbr,
                        long long nbr_stride, int use_gn, float gn_eps, const float* residual, int ld_res, int relu_out,
                        float* out, int ld_out, int precision, void* stream);
/* The weight gradient of that convolution (training; additive within ABI version 9):
 *   grad_w[k, ci, co] = sum over the rows p < M with nbr[k * nbr_stride + p] >= 0 of src[nbr[k, p] * ld_src + ci] * grad_out[p * ld_grad + co]
 * for the forward's table `nbr` ([n_seg, nbr_stride] int32, entries in [-1, n_in): the caller's contract, not checked), its source
 * `src` [n_in, ld_src] (first K columns) and the gradient `grad_out` [M, ld_grad] (first N columns) of its M output rows.
 * grad_w [n_seg, K, N] contiguous (the layout of _SparseConv.kernel): EVERY element is written; a slab whose offset has no present
 * row is exactly 0, and so is everything with M == 0 (src, nbr, grad_out and workspace may then be null).  Exact-fp32 matrix
 * instructions, no float atomics: the row chunks are a function of M alone (512-row blocks, at most 128 chunks), a chunk's partial
 * tile goes to the workspace and the partials are added in chunk order -- two calls return the same bits, on any device.  Source
 * rows no table entry names and columns behind K / N are never read.  No step synchronises with the host.
 * Errors, all before anything is enqueued and with grad_w untouched: V3D_ERR_BAD_SHAPE unless 0 <= M <= 2^30, 1 <= n_seg <= 27, K and N
 * multiples of 16 in [16, 128], ld_src >= K, ld_grad >= N, nbr_stride >= M; V3D_ERR_BAD_ARG for a null pointer, a src / grad_out /
 * grad_w / workspace that is not 16-byte aligned or an ld that is no multiple of 4; V3D_ERR_WORKSPACE_TOO_SMALL.
 * v3d_sparse_conv_weight_grad_workspace_bytes returns 0 for a shape the call refuses (and for M == 0).
 * Developer option "wgrad_compact" (v3d_set_option; 1 | 0, default 1): the kernel stages the present rows of a row chunk only | every
 * row, absent ones as zero rows (the same terms; the groups of four rows the matrix instruction adds differ). */
size_t v3d_sparse_conv_weight_grad_workspace_bytes(int M, int n_seg, int K, int N);
int v3d_sparse_conv_weight_grad_f32(const float* src, int ld_src, const int32_t* nbr, long long nbr_stride, int n_seg,
                                    const float* grad_out, int ld_grad, int M, int K, int N, float* grad_w, void* workspace,
                                    size_t workspace_bytes, void* stream);
int v3d_fill_f32(float* ptr, size_t n, float value, void* stream);
/* PointNet input of PL3DVNet.model_scene (mv3d/lightningmodel.py:180-183): out[i] = [pts[edge_pt[i]] - anchor_pts[edge_anchor[i]]
 * | pts_feat[edge_pt[i]]], out [n_edges, 3 + C]; pts [*, 3], anchor_pts [*, 3], pts_feat [*, C], edges int64. */
int v3d_pointnet_input_f32(const float* pts, const float* anchor_pts, const float* pts_feat, const int64_t* edge_anchor,
                           const int64_t* edge_pt, int n_edges, int C, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sparse-tensor structure (replaces MinkowskiEngine's coordinate manager; semantics: SURVEY.md
 * Appendix A).  coords are int32 [N,4] = (batch, x, y, z), unique rows.
 *   v3d_hash_build        open-addressing table over the coordinate map (buffer >= v3d_hash_bytes(n))
 *   v3d_sparse_neighbors  nbr[k][p] = row of out_coords[p] + step*o_k (or -1), k = (ox+1)+3(oy+1)+9(oz+1);
 *                         conv: step = +tensor_stride_in, transposed conv: step = -tensor_stride_out
 *   v3d_sparse_interp_f32 MinkowskiInterpolation (refinement.py:26,39): trilinear interpolation of
 *                         feats [N,C] at pts [n_pts, n_hyp, 3] (world), query coordinate
 *                         ((p - min_pts[batch]) / res) * tensor_stride, missing corners add 0; result
 *                         written to out[q*ld_out + col0 .. +C); workspace >= v3d_sparse_interp_workspace_bytes.
 * ------------------------------------------------------------------------------------------ */
size_t v3d_hash_bytes(int n);
int v3d_hash_build(const int32_t* coords, int n, void* table, size_t table_bytes, void* stream);
/* Keys pack 16 bits per field: batch in [0, 65535], x/y/z in [-8, 65519].  A row outside that range is left out and
 * sets the table's error word; v3d_hash_status copies it to the host (synchronises) -> V3D_ERR_BAD_SHAPE. */
int v3d_hash_status(const void* table, int n, void* stream);
int v3d_sparse_neighbors(const void* table, int n_in, const int32_t* out_coords, int n_out, int step,
                         int32_t* nbr, void* stream);
size_t v3d_sparse_interp_workspace_bytes(int n_pts, int n_hyp);
int v3d_sparse_interp_f32(const void* table, int n_in, const float* feats, int C, int tensor_stride,
                          const float* pts, const int64_t* pts_batch, int n_pts, int n_hyp,
                          const float* min_pts, float res, float* out, int ld_out, int col0,
                          void* workspace, size_t workspace_bytes, void* stream);
/* The adjoint of v3d_sparse_interp_f32 with respect to feats (training):
 *   grad_feats[r, c] = sum over the corner slots (q, k) with row(q, k) == r of w(q, k) * grad_out[q * ld_grad + col0 + c],
 * row(q, k) and w(q, k) being the forward's corner table (the same kernel fills it).  grad_feats [n_in, C] (16-byte aligned):
 * EVERY element is written, rows nobody touches as +0.  No float atomics: the corner slots are grouped by row (stable) and each
 * row's list is summed in list order, lists of more than 512 slots in chunks of 512 whose partial sums are added in chunk order;
 * the result is bitwise reproducible from call to call.  No step synchronises with the host.  The same C, n_pts * n_hyp * 8 < 2^31
 * and error codes as the forward; ld_grad >= col0 + C; n_pts == 0 zero-fills grad_feats (the workspace may then be null). */
size_t v3d_sparse_interp_backward_workspace_bytes(int n_in, int C, int n_pts, int n_hyp);
int v3d_sparse_interp_backward_f32(const void* table, int n_in, int C, int tensor_stride, const float* pts,
                                   const int64_t* pts_batch, int n_pts, int n_hyp, const float* min_pts, float res,
                                   const float* grad_out, int ld_grad, int col0, float* grad_feats, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Row B3 (mv3d/utils.py:38-64 incl. the un-vendored torch_geometric voxel_grid / torch_cluster grid,
 * restated) and the stride-2 coordinate maps of row B6.  Output sizes are data dependent, so
 * v3d_sort_unique_u64 returns the count to the HOST and synchronises the stream (as torch.unique does
 * in the reference, utils.py:48); everything else is asynchronous.
 *   v3d_voxel_keys       bounding box of pts [n,3] -> ceil-based grid size + trunc+1 cell counts -> 1-D
 *                        voxel id per point (utils.py:39-45); metadata stays in `workspace`
 *   v3d_sort_unique_u64  ascending unique keys (torch.unique, :48)
 *   v3d_lower_bound_u64  position of each point's key in the unique list = inverse index (:48-49)
 *   v3d_voxel_decode     anchor batch, 3-D voxel index, voxel centre, per-batch shift to min 0 (:50-62);
 *                        `workspace` must be the buffer v3d_voxel_keys filled; half_edge = edge_len / 2
 *   v3d_strided_keys / v3d_unpack_coords   packed keys of floor(c / 2ts) * 2ts and back to int32 [n,4]
 * ------------------------------------------------------------------------------------------ */
/* Row B4's max-pooling over the points of a voxel (scenemodeling.py:129-141, torch_scatter.scatter(reduce='max')) without
 * atomics: v3d_segment_csr groups the rows by segment id once (perm [n]: row indices sorted by id, stable; offsets [n_seg+1]),
 * v3d_segment_max_f32 reduces every segment's rows of src [n, ld] to out [n_seg, ld_out] (first N columns; an empty segment
 * yields -inf, the initial value of the atomic version's pool).  Ids must lie in [0, n_seg).  N a multiple of 4 up to 256, ld
 * and ld_out multiples of 4 and >= N (else V3D_ERR_BAD_SHAPE); src and out 16-byte aligned, as its siblings below require (it
 * reads and writes 16 bytes per lane as they do): V3D_ERR_BAD_ARG for a null pointer or a misaligned matrix. */
size_t v3d_segment_csr_workspace_bytes(int n);
int v3d_segment_csr(const int32_t* seg_id, int n, int n_seg, int32_t* perm, int32_t* offsets, void* workspace,
                    size_t workspace_bytes, void* stream);
int v3d_segment_max_f32(const float* src, int ld, const int32_t* perm, const int32_t* offsets, int n_seg, int N, float* out,
                        int ld_out, void* stream);
/* The backward of that pooling and of PointNet's cat(x, pool[idx]) (training; additive within ABI version 9).
 * All three read whole rows 16 bytes per lane through perm / offsets of v3d_segment_csr (or seg_id itself), use no scratch
 * buffer, no LDS and no float atomics, and return the same bits in every call.  Shapes and alignment as v3d_segment_max_f32: N a
 * multiple of 4 up to 256, every ld a multiple of 4 and >= N, every matrix 16-byte aligned.  Of an output's rows the
 * first N columns are written, EVERY one of them; columns behind N and rows behind the last are never touched.
 * Errors, before anything is enqueued: V3D_ERR_BAD_ARG for a null pointer or a misaligned matrix, V3D_ERR_BAD_SHAPE otherwise.
 *   v3d_segment_max_arg_f32  out as v3d_segment_max_f32 (the same bits for every input without NaN) and arg [n_seg, ld_arg]
 *     int32: the ROW of src (not the position in perm) that holds the maximum; among equal values the lowest row (rows ascend
 *     along a segment's list: the sort is stable).  A NaN never wins; an empty segment (and one of NaN rows only) gives -inf
 *     and -1.  This is torch_scatter's rule on the CPU (first on strict >); DESIGN.md 4.1f says what is pinned of it.
 *   v3d_segment_sum_f32  out[s] = (the sum of the rows at the even positions offsets[s], offsets[s] + 2, ... of the list, added
 *     in that order to +0) + (the same for the odd positions): two chains, one final addition.  An empty segment gives +0.
 *   v3d_pointnet_pool_backward_f32  grad_x[r, c] = (x[r, c] > 0 ? grad_lin[r, c] : 0) + (arg[seg_id[r], c] == r ?
 *     grad_pool[seg_id[r], c] : 0) for the n rows r: the ReLU mask of the direct path and the single-winner scatter of the
 *     pooled path in one pass, every element written once.  grad_lin == NULL (x may then be NULL): the second term alone.
 *     seg_id [n] int32 must lie in [0, rows of grad_pool and arg): the caller's contract, not checked. */
int v3d_segment_max_arg_f32(const float* src, int ld, const int32_t* perm, const int32_t* offsets, int n_seg, int N, float* out,
                            int ld_out, int32_t* arg, int ld_arg, void* stream);
int v3d_segment_sum_f32(const float* src, int ld, const int32_t* perm, const int32_t* offsets, int n_seg, int N, float* out,
                        int ld_out, void* stream);
int v3d_pointnet_pool_backward_f32(const float* grad_lin, int ld_lin, const float* x, int ld_x, const int32_t* seg_id,
                                   const float* grad_pool, int ld_pool, const int32_t* arg, int ld_arg, int n, int N,
                                   float* grad_x, int ld_gx, void* stream);
size_t v3d_sort_unique_workspace_bytes(int n);
int v3d_sort_unique_u64(const uint64_t* keys_in, int n, uint64_t* keys_out, int* n_unique_host,
                        void* workspace, size_t workspace_bytes, void* stream);
int v3d_strided_keys(const int32_t* coords, int n, int tensor_stride, uint64_t* keys_out, void* stream);
int v3d_unpack_coords(const uint64_t* keys, int n, int32_t* coords_out, void* stream);
size_t v3d_voxelize_workspace_bytes(void);
int v3d_voxel_keys(const float* pts, const int64_t* pts_batch, int n, float edge_len, uint64_t* keys_out,
                   void* workspace, size_t workspace_bytes, void* stream);
/* Range checks of v3d_voxel_keys (batch ids in [0, 1024), at most 65000 cells per axis, no NaN): the error word lives in
 * `workspace`; this call copies it to the host (synchronises) and returns V3D_ERR_BAD_SHAPE if it is set, in which case
 * v3d_voxel_decode writes nothing. */
int v3d_voxelize_status(const void* workspace, size_t workspace_bytes, void* stream);
int v3d_lower_bound_u64(const uint64_t* sorted_unique, int n_unique, const uint64_t* queries, int n,
                        int64_t* index_out, void* stream);
int v3d_voxel_decode(const uint64_t* unique_keys, int n_unique, float edge_len, float half_edge,
                     float* anchor_pts, int32_t* anchor_idx3d, int64_t* anchor_batch, void* workspace,
                     size_t workspace_bytes, void* stream);

/* Row C2b tail + C3: last Conv1d(C -> 1, k3, pad 1, bias) over the hypothesis axis, softmax
 * (refinement.py:24,43) and optional expectation sum_i p_i*offset_vals_i (lightningmodel.py:238-241).
 * act [n_pts, n_hyp, C]; weight [1, C, 3]; preds [n_pts, n_hyp]; expect [n_pts] or NULL. */
int v3d_decoder_head_f32(const float* act, int n_pts, int n_hyp, int C, const float* weight,
                         const float* bias, const float* offset_vals, float* preds, float* expect,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * SURVEY.md 8f rank 2 -- PropagationNet, the learned 3x3 depth propagation of stage 3
 * (mv3d/subnetworks/upsampling.py:14-36; called at 1/4, 1/2 and full resolution by mv3d/eval-3dvnet.py:101-125 and
 * mv3d/lightningmodel.py:85,98,111).  Replaces PropagationNet.forward(features, depth):
 *   x = cat(features, depth); four Conv2d(3x3, pad 1, no bias) + BatchNorm2d (eval, folded) + ReLU (in -> 32 -> 32 -> 32 -> 9);
 *   p = softmax over the 9 logits; out = sum_k p_k * unfold(replicate_pad(depth))_k.
 * v3d_propagation_pack takes HOST pointers to conv{1..4}.0.weight [Co, Ci, 3, 3] and conv{1..4}.1.{weight, bias,
 * running_mean, running_var}; in_dim = guide channels + 1 (33 for the feature-guided nets, 4 for the image-guided one).
 *   features [B, in_dim - 1, H, W], depth [B, 1, H, W] (= [B, H, W]), out [B, H, W]; `precision` (ABI version 5) =
 *   V3D_PRECISION_SPLIT_BF16 | V3D_PRECISION_FP32 (exact fp32 products on v_mfma_f32_16x16x4_f32, the reference's arithmetic).
 * ------------------------------------------------------------------------------------------ */
typedef struct v3d_propagation_weights v3d_propagation_weights;
int v3d_propagation_pack(const float* const* conv_weight_host, const float* const* bn_weight_host,
                         const float* const* bn_bias_host, const float* const* bn_mean_host,
                         const float* const* bn_var_host, int in_dim, int h_dim, float bn_eps,
                         v3d_propagation_weights** out_handle);
void v3d_propagation_free(v3d_propagation_weights* handle);
/* The network, with the nearest-neighbour resize that precedes every call of stage 3 (F.interpolate(depth, size, 'nearest'),
 * mv3d/eval-3dvnet.py:103,111,119) folded into the kernel's addressing (ABI version 5): depth_lo [B, h0, w0] is the depth BEFORE
 * the resize, iy [H] / ix [W] (DEVICE int32) the source row / column of every output row / column -- the caller obtains them
 * from the host framework's own nearest rule; both NULL with h0 == H, w0 == W = no resize.  One row-marching kernel (csrc/propz.hip):
 * the four layers' activations stay in LDS, no workspace.  (ABI version 7 removed v3d_propagation_f32 and its workspace: this
 * call with null tables does the same job.) */
int v3d_propagation_up_f32(const v3d_propagation_weights* handle, const float* features, const float* depth_lo, int B, int Cf,
                           int H, int W, int h0, int w0, const int32_t* iy, const int32_t* ix, float* out, int precision, void* stream);

/* Rows C2a + C2b + C3 fused: MinkowskiInterpolation of the three U-Net levels at the hypothesis
 * points (mv3d/subnetworks/refinement.py:28-41) -> the three Conv1d+BN+ReLU layers along the hypothesis axis (:16-23) ->
 * Conv1d(128 -> 1) + softmax (:24,43) -> expected offset (mv3d/lightningmodel.py:237-241): one index kernel (the 8 lattice
 * corners of every hypothesis point on the three levels -> (row, weight) pairs in `workspace`) and ONE matrix kernel; the
 * [n_pts, C, n_hyp] feature tensor and the intermediate activations never reach HBM.  Split-bf16 MFMA operands
 * (V3D_PRECISION_SPLIT_BF16; for exact fp32 use v3d_sparse_interp_f32 + v3d_gemm_gather_f32 + v3d_decoder_head_f32).
 *   layers_host   3 handles from v3d_gemm_pack: Conv1d weights [128, Cin, 3] (strides 1, 3*Cin, 3; n_seg 3) with the folded
 *                 BatchNorm scale / bias; Cin = sum of the level widths + c_feat for the first, 128 for the others
 *   level_*_host  HOST arrays of 3 entries in feature-row order (finest level first, refinement.py:41): hash table
 *                 (v3d_hash_build) and its row count, feats [N, C] (C a multiple of 16, 16-byte aligned, N*C*4 < 2 GB), tensor
 *                 stride, per-batch minimum point [n_batch, 3] (refinement.py:33), x.res
 *   pts [n_pts, n_hyp, 3], pts_batch [n_pts] int64, pts_feat [n_pts, n_hyp, c_feat] or NULL (c_feat 0 or a multiple of 16),
 *   n_hyp <= 8; head_weight [1, 128, 3], head_bias [1]; offset_vals [n_hyp] or NULL; preds [n_pts, n_hyp]; expect [n_pts] or NULL
 *   depth_inout   [n_pts] or NULL: the expected offset is also ADDED to it in place (the driver's `depth += offset`,
 *                 mv3d/eval-3dvnet.py:99: one elementwise launch less per sweep)
 *   workspace     v3d_decoder_fused_workspace_bytes(n_pts, n_hyp) bytes, 16-byte aligned (ABI version 3) */
size_t v3d_decoder_fused_workspace_bytes(int n_pts, int n_hyp);
int v3d_decoder_fused_f32(const v3d_gemm_weights* const* layers_host, const float* head_weight, const float* head_bias,
                          const void* const* level_table_host, const int* level_n_host,
                          const float* const* level_feats_host, const int* level_C_host, const int* level_stride_host,
                          const float* const* level_min_pts_host, const float* level_res_host, const float* pts,
                          const int64_t* pts_batch, const float* pts_feat, int c_feat, int n_pts, int n_hyp,
                          const float* offset_vals, float* preds, float* expect, float* depth_inout, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * SURVEY.md 8f rank 3 -- the 2D feature extractor of MVSNet (mv3d/subnetworks/mvsnet.py:55-105: torchvision MnasNet-1.0 trunk +
 * FeaturePyramidNetwork): the layer kernels on CHANNELS-LAST fp32 activations [n, H, W, C] (C a multiple of 8), eval-mode
 * BatchNorm folded into weights / bias by the caller (3dvnet_amd/backbone.py drives them with torchvision's key names).
 *   v3d_conv_pack        HOST weight [Cout, K], K = taps * Cin in (tap, channel) order (Conv2d weight permuted to
 *                        [Cout, kh, kw, Cin]), bias [Cout] or NULL -> handle (exact-fp32 MFMA fragments)
 *   v3d_conv_nhwc_f32    1x1 (taps 1) or 3x3 / pad 1 (taps 9) convolution + bias (+ ReLU) (+ residual: res_mode 1 = res
 *                        [n, H, W, Cout]; 2 = nearest-upsampled res [n, ceil(H/2), ceil(W/2), Cout], the FPN's top-down addition; odd H, W allowed)
 *   v3d_depthwise_nhwc_f32  k x k (3 | 5) depthwise, pad k/2, stride 1 | 2, DEVICE w [k*k][C], bias [C] -> [n, ceil(H/s), ceil(W/s), C]
 *   v3d_stem_f32         Conv2d(3 -> 32, k3, s2, p1) + bias + ReLU from the NCHW image; DEVICE w [27][32] ((c, ky, kx) major)
 *   v3d_nhwc_to_nchw_f32 [n, HW, C] -> [n, C, HW] (C a multiple of 32): the layout the cost-volume entry points take
 * ------------------------------------------------------------------------------------------ */
typedef struct v3d_conv_weights v3d_conv_weights;
int v3d_conv_pack(const float* w_host, const float* bias_host, int cout, int k, v3d_conv_weights** out_handle);
void v3d_conv_free(v3d_conv_weights* handle);
int v3d_conv_nhwc_f32(const v3d_conv_weights* handle, const float* x, int n, int H, int W, int cin, int taps, int relu,
                      int res_mode, const float* res, float* out, void* stream);
int v3d_depthwise_nhwc_f32(const float* x, const float* w, const float* bias, int n, int H, int W, int C, int ksize, int stride,
                           int relu, float* out, void* stream);
int v3d_stem_f32(const float* image, const float* w, const float* bias, int n, int H, int W, float* out, void* stream);
int v3d_nhwc_to_nchw_f32(const float* in, float* out, int n, int C, int HW, void* stream);

/* An inverted-residual block of the trunk (torchvision mnasnet._InvertedResidual: 1x1 expand + BN + ReLU -> k x k depthwise,
 * stride s, + BN + ReLU -> 1x1 project + BN, + x when `residual`) as ONE kernel (csrc/irb.hip; ABI version 6, round 6): the
 * expanded tensor never reaches HBM.  Split-bf16 matrix operands, fp32 depthwise taps; the exact-fp32 block is the three calls above.
 *   v3d_irb_pack       HOST weights with BatchNorm folded: w_expand [mid, cin], w_dw [mid, k, k], w_project [cout, mid], biases
 *                      [mid], [mid], [cout]; cin, mid, cout multiples of 8; k 3 | 5; stride 1 | 2; residual needs cin == cout, stride 1
 *   v3d_irb_supported  1 when a kernel instance exists for this block at input size H x W (the MnasNet-1.0 blocks at image sides
 *                      that are multiples of 32 and at 240 x 320), else 0: the caller then runs the three-call path
 *   v3d_irb_nhwc_f32   x [n, H, W, cin] -> out [n, ceil(H / s), ceil(W / s), cout], channels-last fp32; `workspace` of
 *                      v3d_irb_workspace_bytes(handle, n, H, W) bytes (16-byte aligned; 0 bytes / NULL for most maps): a map with fewer
 *                      tiles than the chip has CUs (71 images at 1/32 resolution) shares a tile's expanded channels out over several
 *                      workgroups whose partial sums meet there, summed in a fixed order by a second launch */
typedef struct v3d_irb_weights v3d_irb_weights;
int v3d_irb_pack(const float* w_expand, const float* b_expand, const float* w_dw, const float* b_dw, const float* w_project,
                 const float* b_project, int cin, int mid, int cout, int ksize, int stride, int residual,
                 v3d_irb_weights** out_handle);
void v3d_irb_free(v3d_irb_weights* handle);
int v3d_irb_supported(const v3d_irb_weights* handle, int H, int W);
/* The trunk's first three layers (mnasnet layers 0-7: 3x3 / stride 2 convolution 3 -> 32 + BN + ReLU, 3x3 depthwise + BN + ReLU, 1x1 -> 16
 * + BN) as the same kernel: the 27 (channel, ky, kx) taps of the first convolution are the K dimension of its first matrix product.
 *   v3d_stem_block_pack  HOST w_stem [32, 27] (Conv2d weight [32, 3, 3, 3] flattened), w_dw [32, 3, 3], w_pw [16, 32], BatchNorm folded
 *   v3d_stem_block_f32   image [n, 3, IH, IW] (NCHW, even sides) -> out [n, IH/2, IW/2, 16] channels-last; free with v3d_irb_free */
int v3d_stem_block_pack(const float* w_stem, const float* b_stem, const float* w_dw, const float* b_dw, const float* w_pw,
                        const float* b_pw, v3d_irb_weights** out_handle);
int v3d_stem_block_f32(const v3d_irb_weights* handle, const float* image, int n, int IH, int IW, float* out, void* stream);
size_t v3d_irb_workspace_bytes(const v3d_irb_weights* handle, int n, int H, int W);
int v3d_irb_nhwc_f32(const v3d_irb_weights* handle, const float* x, int n, int H, int W, float* out, void* workspace,
                     size_t workspace_bytes, void* stream);


/* One level of the feature pyramid (torchvision FeaturePyramidNetwork, mvsnet.py:83-105) as ONE kernel (csrc/fpn.hip; ABI version 6):
 * inner = lateral 1x1 (x) + bias + nearest-upsampled inner of the coarser level; out = 3x3 / pad 1 (inner) + bias, written in the
 * reference layout.  feat_dim 32, cin a multiple of 8 and <= 48 (the levels at 1/2, 1/4, 1/8); split-bf16 matrix operands.
 *   v3d_fpn_pack       HOST w_lateral [32, cin], b_lateral [32], w_out [32, 32, 3, 3], b_out [32]
 *   v3d_fpn_level_f32  x [n, H, W, cin] channels-last; coarse_inner [n, ceil(H/2), ceil(W/2), 32] channels-last or NULL;
 *                      inner_out [n, H, W, 32] channels-last or NULL (not needed for the finest level); out [n, 32, H, W] */
typedef struct v3d_fpn_weights v3d_fpn_weights;
int v3d_fpn_pack(const float* w_lateral, const float* b_lateral, const float* w_out, const float* b_out, int cin,
                 v3d_fpn_weights** out_handle);
void v3d_fpn_free(v3d_fpn_weights* handle);
int v3d_fpn_level_f32(const v3d_fpn_weights* handle, const float* x, const float* coarse_inner, int n, int H, int W,
                      float* inner_out, float* out, void* stream);

/* Multi-view depth fusion (csrc/fusion.hip; ABI version 8): the depth maps of a scene -> a fused point cloud with the semantics of
 * mv3d/eval/pointcloudfusion_custom.py (process_depth :10-95, process_scene :98-116), the step mv3d/eval/processresults.py:276
 * runs on the preds.npz record.  Pixel (x, y) of reference view r with depth d is lifted to X = P_r^-1 (K_r^-1 [x d, y d, d]);
 * for each source s in list order q = K_s (R_s X + t_s), (u, v) = q_xy / q_z; the source is valid when q_z > 1e-4, 0 <= u <= w-1,
 * 0 <= v <= h-1 and |q_z - z_s| < z_thresh, z_s = the nearest texel of d_s (grid_sample nearest / align_corners / zero padding);
 * a valid source adds X_s = R_s^T (K_s^-1 [u z_s, v z_s, z_s] - t_s).  pts = (X + sum X_s) / (n_valid + 1), fp32, list order.
 *   v3d_fusion_workspace_bytes  scratch of both calls for n_img maps of h x w (0 for sizes the calls reject); calls issued on one
 *                         stream may share one workspace
 *   v3d_fuse_depths_f32   depths [n_img, h, w]; cams [n_img, 48] camera blocks: [0..8] K, [9..17] K^-1, [18..26] R, [27..29] t,
 *                         [30..41] rows 0..2 of P^-1 (3 x 4, row major), [42..47] unused -- the inverses come from the caller
 *                         (torch.inverse) so that their last bits are the reference's.  ref_img_host [n_ref] (HOST) = image index
 *                         of every reference, NULL = all n_img images (n_ref == n_img).  edge_ofs_host [n_ref + 1] / edge_src_host
 *                         (HOST, CSR as in v3d_psv_variance_*): the source list of every reference, at most n_img^2 entries; both
 *                         NULL = all other images in ascending order.  The lists are checked here and copied to the workspace on
 *                         `stream` with hipMemcpyAsync: from ordinary (pageable) host memory the runtime has taken its copy when the
 *                         call returns and the arrays may be released; arrays in PINNED host memory must stay unchanged until the
 *                         stream has passed the call.  -> pts [n_ref, h w, 3], n_valid [n_ref, h w] int32, dense, every element written.
 *                         Errors: V3D_ERR_BAD_SHAPE for h or w < 2 (the normalisation divides by w - 1) and bad counts,
 *                         V3D_ERR_BAD_ARG for a reference / source index outside [0, n_img) or a malformed list.
 *   v3d_fusion_compact    keep = n_valid >= n_consistent_thresh -> all_valid [n_ref, h, w] bytes, view_count [n_ref], view_ofs
 *                         [n_ref + 1] (exclusive scan), the kept points out_pts [*, 3] and colours out_rgb [*, px_bytes] in (view,
 *                         row-major pixel) order, their number in the device word `total`.  images [n_ref, h w, px_bytes] = the
 *                         references' colours, px_bytes bytes per pixel of any type (NULL with out_rgb NULL: points only);
 *                         out_pts / out_rgb hold n_ref h w entries (the worst case).  Stable and atomic-free: bit-identical
 *                         across launches. */
size_t v3d_fusion_workspace_bytes(int n_img, int h, int w);
int v3d_fuse_depths_f32(const float* depths, const float* cams, int n_img, int h, int w, const int32_t* ref_img_host, int n_ref,
                        const int32_t* edge_ofs_host, const int32_t* edge_src_host, double z_thresh, float* pts, int32_t* n_valid,
                        void* workspace, size_t workspace_bytes, void* stream);
int v3d_fusion_compact(const int32_t* n_valid, const float* pts, const void* images, int px_bytes, int n_ref, int h, int w,
                       int n_consistent_thresh, uint8_t* all_valid, int32_t* view_count, int32_t* view_ofs, float* out_pts,
                       void* out_rgb, int32_t* total, void* workspace, size_t workspace_bytes, void* stream);

/* Scoring of a fused point cloud (csrc/cloudmetrics.hip; ABI version 9): the three steps mv3d/eval/processresults.py:283-295 runs
 * on the fused cloud -- voxel down-sample, nearest neighbours in both directions (mv3d/eval/metricfunctions.py:102-124), the five
 * numbers of eval_mesh (:70-99).
 *   v3d_cloud_downsample_f32  Open3D's VoxelDownSample as documented (restated; not pinned against the package).  pts [n, 3] fp32;
 *                         the rows in use are the first min(max(*n_dev, 0), n) when n_dev (a DEVICE int32 word, e.g. the `total` of
 *                         v3d_fusion_compact) is given, else all n.  vmin = double(min over rows) - voxel_size / 2, cell =
 *                         floor((double(p) - vmin) / voxel_size) per axis, key = x 2^42 + y 2^21 + z.  Output row of a cell = the
 *                         double-precision mean of its member rows, summed in original row order, rounded once to fp32; attr
 *                         [n, n_attr] (NULL with n_attr 0) is averaged the same way.  Output order: ascending key.  out_pts
 *                         [n, 3] / out_attr [n, n_attr] hold n rows (the worst case); the number of cells lands in the DEVICE word
 *                         out_count.  Data-dependent errors never fail the call: they set out_count to the NEGATED error bits
 *                         (1 non-finite coordinate, 2 extent / voxel_size >= 2^21 on an axis, 4 voxel_size not positive and
 *                         finite) and are reported by v3d_cloud_status.  No atomics: bit-identical across launches.
 *   v3d_cloud_status      reads the status of the last down-sample call on this workspace (synchronises the stream): returns
 *                         V3D_OK and the number of output rows in *n_out_host (HOST, may be NULL), or V3D_ERR_BAD_ARG (bits 1, 4) /
 *                         V3D_ERR_BAD_SHAPE (bit 2) with *n_out_host = 0.
 *   v3d_nn_query_f32      for every query row the nearest target row: idx [n_query] = its index in the target's own row order,
 *                         dist [n_query] = sqrt(dx^2 + dy^2 + dz^2) evaluated in fp32 from fp32 differences.  Exact (no radius, no
 *                         approximation) and deterministic: the result is the minimum of (fp32 distance, target row).  The search
 *                         index (Morton-sorted copy of the target, cell table) is built in the workspace by every call.
 *                         n_query == 0: nothing is done; n_target == 0: idx = -1, dist = +inf.  Coordinates must be finite (a NaN
 *                         row is never a neighbour and finds none).
 *   v3d_cloud_metrics_f64 dist_pred [n_pred] = distance of every predicted row to the target cloud, dist_target [n_target] = of
 *                         every target row to the predicted cloud -> out [5] doubles (DEVICE): acc = mean(dist_pred), comp =
 *                         mean(dist_target), prec / recal = share of double(d) < threshold in dist_pred / dist_target, fscore =
 *                         2 prec recal / (prec + recal + 1e-8).  Double sums in a fixed two-stage order.  An empty array gives
 *                         NaN, as the reference's NumPy means do.
 * Host-side errors (returned before anything is enqueued): null pointers, negative counts, a too-small workspace,
 * threshold <= 0. */
size_t v3d_cloud_downsample_workspace_bytes(int n);
int v3d_cloud_downsample_f32(const float* pts, const float* attr, int n_attr, int n, const int32_t* n_dev, double voxel_size,
                             float* out_pts, float* out_attr, int32_t* out_count, void* workspace, size_t workspace_bytes,
                             void* stream);
int v3d_cloud_status(const void* workspace, size_t workspace_bytes, int32_t* n_out_host, void* stream);
size_t v3d_nn_workspace_bytes(int n_target, int n_query);
int v3d_nn_query_f32(const float* target, int n_target, const float* query, int n_query, int32_t* idx, float* dist,
                     void* workspace, size_t workspace_bytes, void* stream);
size_t v3d_cloud_metrics_workspace_bytes(void);
int v3d_cloud_metrics_f64(const float* dist_pred, int n_pred, const float* dist_target, int n_target, double threshold,
                          double* out, void* workspace, size_t workspace_bytes, void* stream);

/* TSDF integration of depth maps (csrc/tsdf.hip): the semantics of mv3d/eval/tsdf_atlas.py TSDFFusion.integrate (:390-443) and
 * get_tsdf (:453-463), the volume mv3d/eval/processresults.py:359-382 builds from the preds.npz record.  ABI version: STILL 9.
 * These two entry points are purely additive -- new symbols, no changed signature -- so a caller built against version 9 keeps
 * working and v3d_version() is not bumped.
 *   v3d_tsdf_integrate_f32  applies n views, in the given order, to a volume of nx x ny x nz voxels, IN PLACE (a fresh volume, one
 *                         view at a time, or a scene in chunks).  State, flat index (x ny + y) nz + z: tsdf [nx ny nz] = the running
 *                         sum (fresh: -1, after the reference's reset(): +1), weight [nx ny nz] (fresh: 0), color [3, nx ny nz]
 *                         (fresh: 0; NULL together with images: no colour).  voxel_size, trunc_margin and origin [3] (HOST, read
 *                         before the call returns) are taken as fp32.  projections [n, 12] (DEVICE) = the 3 x 4 matrices K [R | t],
 *                         row major; depths [n, h, w]; images [n, 3, h, w] fp32.  Per voxel and view, all fp32: world = fl(fl(i *
 *                         voxel_size) + origin) per axis; c_r = row r of P . [world; 1] as a k-ordered FMA chain; (px, py) =
 *                         round-half-even(c0 / c2, c1 / c2); valid = px >= 0, py >= 0, px < w, py < h, c2 > 0 (decided on the
 *                         floats: a NaN or huge coordinate is invalid), d = depths[py, px] > 0, dist = min((d - c2) / trunc_margin,
 *                         1) > -1; a valid view sets tsdf = dist when weight == 0, else tsdf += dist; weight += 1; color[c] +=
 *                         images[c, py, px].  No atomics; one call of n views gives the bits of n calls of one view.  n == 0:
 *                         nothing is done.
 *   v3d_tsdf_normalize_f32  tsdf_out = tsdf_sum / weight where weight > 0, tsdf_sum elsewhere; color_out [3, n_vox] likewise from
 *                         color_sum (both NULL: no colour).
 * Both are asynchronous on `stream`, allocate nothing and never synchronise.  Host-side errors: V3D_ERR_BAD_ARG for a null
 * pointer, a voxel size or truncation margin that is not positive and finite, images without a colour volume (or the reverse);
 * V3D_ERR_BAD_SHAPE for a count that is not positive or nx ny nz >= 2^31. */
int v3d_tsdf_integrate_f32(float* tsdf, float* weight, float* color, int nx, int ny, int nz, double voxel_size,
                           const float* origin_host, double trunc_margin, const float* projections, const float* depths,
                           const float* images, int n, int h, int w, void* stream);
int v3d_tsdf_normalize_f32(const float* tsdf_sum, const float* weight, const float* color_sum, int n_vox, float* tsdf_out,
                           float* color_out, void* stream);

/* Triangle meshes from TSDF volumes (csrc/mesh.hip): marching cubes with the project's own case table (csrc/mc_table.h, generated
 * from a rule by scripts/gen_mc_table.py) and what mv3d/eval/tsdf_atlas.py does around its marching-cubes call.  ABI version:
 * STILL 9 (additive, as the TSDF symbols are).
 *   Volume: tsdf [nx, ny, nz] fp32, z fastest (flat index (x ny + y) nz + z), as v3d_tsdf_normalize_f32 leaves it; values are
 *   clamped to [-1, 1] on load (a NaN stays a NaN).  A voxel is inside iff its clamped value is < 0 (NaN and -0.0: outside).
 *   color [3, nx ny nz] fp32 (may be NULL).
 *   Vertices: one per sign-changing grid edge, ordered by the owning voxel's flat index, then by axis x, y, z (a voxel owns the
 *   edges that leave it in +x, +y, +z and stay inside the volume).  For the edge from voxel a to its +axis neighbour b, all fp32:
 *   t = va / (va - vb), index coordinate = fl(i + t), world = fl(fl(index * voxel_size) + origin).
 *   Triangles: ordered by the flat index of the cell's lowest voxel, then in table order; indices into the FINAL vertex list.
 *   mode V3D_MESH_MODE_MESH = TSDF.get_mesh (:161-253): a vertex is BAD when, among the eight clamped values at floor(index
 *     coordinate) + {0, 1}^3 (clipped to the volume), one equals +1 and one equals -1; bad vertices and every triangle that
 *     references one are dropped, the rest is renumbered in order.  Colour = color[:, round-half-even(index coordinate)] clamped
 *     to [0, 255], truncated to a byte, stored in channel order [2, 1, 0].  Empty-mesh rule: no vertex and no triangle when the
 *     minimum of the clamped volume is >= 0 or its maximum is <= 0.
 *   mode V3D_MESH_MODE_POINT_CLOUD = the tsdf_point_cloud attribute of get_tsdf (:465-481): every vertex, no triangles, no
 *     empty-mesh rule; colour = floor(color[:, round(index coordinate)]) as a byte, channel order [0, 1, 2].
 * Two calls, and ONE read-back between them:
 *   v3d_mesh_count_f32    classifies the volume in `workspace` (v3d_mesh_workspace_bytes) and writes the number of vertices and
 *                         triangles to the DEVICE words counts[0], counts[1] (both -1 when a total reaches 2^31).  The caller
 *                         reads the two words to size the outputs.
 *   v3d_mesh_extract_f32  with the SAME volume, mode and workspace, untouched since the count call: writes verts [v_cap, 3] fp32,
 *                         colors [v_cap, 3] bytes (NULL exactly when color is NULL) and tris [f_cap, 3] int32.  v_cap / f_cap are
 *                         the rows the outputs hold, normally the two counts; rows beyond a capacity are not written (no status
 *                         word: the counts are known).  A capacity of 0 skips that output.  origin [3] and voxel_size are taken
 *                         as fp32 (origin: HOST, read before the call returns).
 * Both are asynchronous on `stream`, allocate nothing and never synchronise; no atomics, so repeated calls give identical bits.
 * Host-side errors: V3D_ERR_BAD_ARG for a null required pointer, an unknown mode, a voxel size that is not positive and finite,
 * a colour volume without a colour output (or the reverse); V3D_ERR_BAD_SHAPE for a dimension that is not positive, nx ny nz >=
 * 2^31 or a negative capacity; V3D_ERR_WORKSPACE_TOO_SMALL. */
#define V3D_MESH_MODE_MESH 0
#define V3D_MESH_MODE_POINT_CLOUD 1
size_t v3d_mesh_workspace_bytes(int nx, int ny, int nz);
int v3d_mesh_count_f32(const float* tsdf, int nx, int ny, int nz, int mode, int32_t* counts, void* workspace,
                       size_t workspace_bytes, void* stream);
int v3d_mesh_extract_f32(const float* tsdf, const float* color, int nx, int ny, int nz, double voxel_size,
                         const float* origin_host, int mode, float* verts, uint8_t* colors, int v_cap, int32_t* tris, int f_cap,
                         const void* workspace, size_t workspace_bytes, void* stream);

/* Depth maps of a triangle mesh (csrc/meshrender.hip): what mv3d/eval/meshtodepth.py (Renderer / process_scene) gets from pyrender
 * -- the depth of the nearest surface along the camera axis at every pixel, 0 where nothing is seen -- as a rasteriser with pinned
 * fp32 arithmetic.  ABI version: STILL 9 (additive, as the TSDF and mesh symbols are).
 *   Inputs (DEVICE): verts [n_vert, 3] fp32 world coordinates; tris [n_tri, 3] int32; projections [n_view, 12] fp32 = the 3 x 4
 *   matrices K [R | t], row major (world -> camera poses, as v3d_tsdf_integrate_f32 takes them).  pixel_center, znear, zfar are
 *   taken as fp32.  Output: depth [n_view, h, w] fp32; status: one int32 DEVICE word.
 *   Pixel (r, c) samples the image-plane point (px, py) = (fl(c + pixel_center), fl(r + pixel_center)) in the coordinates of K
 *   (u = fx X / Z + cx).  pixel_center = 0.5 is OpenGL's sample position, 0 the integer-centre convention of the TSDF kernel.
 *   Per view and triangle, all fp32, every operation rounded on its own (no contraction) except the projection chain:
 *     q_i = P . [X_i; 1] for the three vertices, each row a k-ordered FMA chain whose homogeneous term is a rounded addition (the
 *           function of v3d_tsdf_integrate_f32); q_i.z is the camera depth of the vertex;
 *     A_0 = q_1 x q_2, A_1 = q_2 x q_0, A_2 = q_0 x q_1, each component fl(fl(a b) - fl(c d)) in the usual order
 *           (y z' - z y', z x' - x z', x y' - y x');
 *     det = fl(fl(fl(q_0.x A_0.x) + fl(q_0.y A_0.y)) + fl(q_0.z A_0.z));
 *     per pixel e_i = fl(fl(fl(A_i.x px) + fl(A_i.y py)) + A_i.z), s = fl(fl(e_0 + e_1) + e_2);
 *     the pixel has a fragment iff (e_0 >= 0 and e_1 >= 0 and e_2 >= 0 and s > 0) or (e_0 <= 0 and e_1 <= 0 and e_2 <= 0 and
 *     s < 0), and z = det / s (IEEE division) satisfies znear <= z <= zfar (a NaN fails).
 *   depth = the smallest z of any fragment at the pixel, 0 where there is none.  This is homogeneous rasterisation: both sides of a
 *   triangle are seen; a triangle that crosses the near plane or the camera plane needs no geometric clipping (the range test is
 *   the clip, per fragment); the inclusive edge rule leaves no crack along a shared edge.  Coverage is this predicate, whatever
 *   way the kernel walks the image, with two rejections that exact arithmetic implies and the kernel takes on the fp32 values: a
 *   triangle whose three q_i.z are all < znear has no fragment (z is a convex combination of them), and a triangle whose three
 *   q_i.z are all >= znear has none outside the bounding box of its three (q.x / q.z, q.y / q.z) widened by one pixel.
 *   Skipped triangles: one with an index outside [0, n_vert) sets bit value 1 of *status, one with a non-finite vertex coordinate
 *   bit value 2; the other triangles are rendered as if those were absent.  *status is 0 after a clean call.
 * The minimum is taken on the bits of z (positive floats order as their bit patterns) with 32-bit atomics, so the output does not
 * depend on scheduling: repeated calls, n views in one call or n calls of one view, and any "render_coop" give identical bits.
 * Asynchronous on `stream`; no workspace, no allocation, no synchronisation.  Host-side errors: V3D_ERR_BAD_ARG for a null
 * pointer, a parameter that is not finite, znear outside (0, zfar); V3D_ERR_BAD_SHAPE for a count or size that is not positive or
 * n_view h w >= 2^31. */
#define V3D_RENDER_STATUS_BAD_INDEX 1
#define V3D_RENDER_STATUS_NON_FINITE 2
int v3d_mesh_render_depth_f32(const float* verts, int n_vert, const int32_t* tris, int n_tri, const float* projections, int n_view,
                              int h, int w, double pixel_center, double znear, double zfar, float* depth, int32_t* status,
                              void* stream);

/* Resampling of a TSDF volume onto another grid (csrc/tsdf_resample.hip): the semantics of mv3d/eval/tsdf_atlas.py TSDF.transform
 * (:255-338) -- crop / pad to another voxel_dim and origin and / or apply a 3 x 4 transform; the first step of eval_tsdf
 * (mv3d/baselines/atlas/evaluation.py:24-51).  ABI version: STILL 9 (additive, as the TSDF, mesh and render symbols are).
 *   Volumes (DEVICE), z fastest: source [sx, sy, sz] at src_origin, output [nx, ny, nz] at dst_origin, both with voxel_size;
 *   channel c of a [C, ...] volume starts at c * (number of voxels).  src_origin [3], dst_origin [3] and matrix [12] (3 x 4, row
 *   major, maps OUTPUT world coordinates to SOURCE world coordinates) are HOST arrays read before the call returns; voxel_size is
 *   taken as fp32.
 *   Per output voxel (ix, iy, iz) and axis a with source size D_a, all fp32, every operation rounded on its own unless stated:
 *     world_a = fl(fl(i_a * voxel_size) + dst_origin_a)                       (the function of v3d_tsdf_integrate_f32)
 *     t_a     = row a of matrix . [world; 1], a k-ordered FMA chain whose homogeneous term is a rounded addition (dot4h_chain)
 *     c_a     = fl(fl(t_a - src_origin_a) / voxel_size)                       (IEEE division)
 *     g_a     = fl(fl(fl(2 c_a) / (D_a - 1)) - 1)                             grid_sample's normalised coordinate
 *     u_a     = fl(fl(fl(g_a + 1) / 2) * (D_a - 1))                           align_corners != 0
 *             = fl(fl(fl(fl(g_a + 1) * D_a) - 1) / 2)                         align_corners == 0 (the reference's default)
 *     outside = some |g_a| >= 1 (a NaN is not outside).
 *   Nearest: r_a = round-half-even(u_a); in bounds iff 0 <= r_a <= D_a - 1 on every axis, decided on the floats before any integer
 *   conversion (a NaN or huge value is out of bounds); out of bounds gives 0 (zero padding).
 *   Trilinear: f_a = floor(u_a), per axis w0_a = fl(fl(f_a + 1) - u_a) at f_a and w1_a = fl(u_a - f_a) at f_a + 1; tap weight =
 *   fl(fl(w_z * w_y) * w_x); value = the sum over the taps inside the volume (same float test) of fl(src * weight), accumulated
 *   from 0 in the order x outermost, z innermost, every addition rounded (no FMA): the order and roundings of torch's CPU
 *   grid_sample.  Taps outside contribute nothing.
 *   v3d_tsdf_resample_f32  ONE launch: the tsdf (tsdf_src -> tsdf_dst, both NULL: skipped) and `channels` fp32 channels (attr_src
 *                         [C, sx, sy, sz] -> attr_dst [C, nx, ny, nz], both NULL with channels == 0) from one coordinate.  tsdf rule
 *                         (:299-314): v = nearest; if |v| < 1, v = trilinear; if outside, v = 1.  Channels: trilinear, nothing else.
 *                         The result of either part does not depend on whether the other is present.
 *   v3d_volume_resample_nearest  `channels` channels of elements of elem_bytes = 1, 2, 4 or 8 bytes, copied in their own type
 *                         (never through fp32): nearest, zero padding (all-zero bytes).  fill_outside = 1: where the voxel is outside,
 *                         the elem_bytes bytes at fill_host (HOST) are written instead (the reference's semseg = -1 and mask_outside
 *                         = True); 0: fill_host is not read.
 * Asynchronous on `stream`; no workspace, no allocation, no atomics, no synchronisation; repeated calls give identical bits.
 * Host-side errors, before any launch: V3D_ERR_BAD_ARG for a null required pointer (or one half of a src / dst pair), a voxel size
 * that is not positive and finite, an origin or matrix entry that is not finite, an elem_bytes or fill_outside outside its set, a
 * source that overlaps a destination; V3D_ERR_BAD_SHAPE for a source size < 2 (the normalisation divides by D - 1), an output
 * size < 1, 2^31 or more voxels on either side, channels < 0 (< 1 for the nearest call). */
int v3d_tsdf_resample_f32(const float* tsdf_src, const float* attr_src, int channels, int sx, int sy, int sz, double voxel_size,
                          const float* src_origin_host, const float* matrix_host, int align_corners, int nx, int ny, int nz,
                          const float* dst_origin_host, float* tsdf_dst, float* attr_dst, void* stream);
int v3d_volume_resample_nearest(const void* src, int elem_bytes, int channels, int sx, int sy, int sz, double voxel_size,
                                const float* src_origin_host, const float* matrix_host, int align_corners, int nx, int ny, int nz,
                                const float* dst_origin_host, int fill_outside, const void* fill_host, void* dst, void* stream);

/* 2D depth metrics of predicted depth maps (csrc/depthmetrics.hip on csrc/depth2d.h): mv3d/eval/metricfunctions.py:26-67 (calc_2d_depth_metrics) as
 * mv3d/eval/processresults.py:153-169 reaches it (nearest-enlarged predictions, valid = pred != 0 & ~isinf(pred)), in one pass
 * over the ground truth and without a temporary.  ABI version: STILL 9 -- two new symbols, nothing changed.
 *   pred [n, hp, wp] fp32; gt [n, H, W] of gt_type 0 (uint16 millimetres), 1 (fp32 metres) or 2 (fp64 metres), aligned to its own
 *   element only; row_src [H], col_src [W] (DEVICE, int32): the row / column of the prediction that ground-truth row r / column c
 *   is scored against (the index tables of a nearest resize; entries are clamped to the prediction); both NULL = identity, then
 *   hp == H and wp == W.  valid_mode 0: every prediction is valid; 1: pred_valid [n, H, W] bytes, non-zero = valid; 2: derived.
 * Per pixel (i, r, c), float64 with every operation rounded on its own and IEEE division, except where noted:
 *   g = double(u16) / 1000.0 | the widened fp32 | the fp64;  pf = pred[i, row_src[r], col_src[c]],  p = double(pf);
 *   pv = true | pred_valid != 0 | (pf != 0 and pf is not +-inf: a NaN prediction is "valid", as in the reference);
 *   m = pv and g >= 0.5 and g < 65.0;  n_pv += pv;  n_m += m;  and only where m holds:
 *   e = |p - g|;  q = g + 1e-7;  S_rel += e / q;  S_diff += e;  S_sqrel += (e e) / q;  S_sq += e e;
 *   t = |double(1.0f / pf) - 1 / g|, the first quotient ONE FP32 DIVISION (the reference's prediction is a float32 tensor where it
 *   writes 1. / depth_pred; everywhere else the float64 ground truth promotes it first);  S_inv += t, a non-finite t counts as 0;
 *   c1 += p / g < 1.25 and g / p < 1.25 (the maximum of the two below the bound; a NaN in either counts nothing); c2, c3 likewise
 *   with 1.5625 and 1.953125.
 * Per image, the reference's mixed types: denom32 = float(n_m) + 1e-7f (one fp32 addition: 1e-7f for an empty mask, 1 + 2^-23 for
 * one pixel, n_m otherwise), denom = double(denom32);
 *   per_image [n, 9] = perc_valid = float(n_pv) / float(H W) (fp32 division), abs_rel = S_rel / denom, abs_diff = S_diff / denom,
 *   abs_inv = S_inv / denom, sq_rel = S_sqrel / denom, rmse = sqrt(S_sq / denom), d_125 = float(c1) / denom32 (fp32 division),
 *   d_125_2, d_125_3 likewise; the fp32 values are stored widened.  counts [n, 5] = n_pv, n_m, c1, c2, c3.
 *   mean [9] = the float64 sum of the rows of per_image in image order, divided by n.
 * Deviation from the reference: a pixel outside m contributes nothing.  The reference multiplies by a 0 / 1 mask, so one masked
 * infinite prediction or NaN ground truth turns its sums into NaN; this call returns the metric over the valid pixels.  Non-finite
 * values inside m propagate by IEEE rules, as there.
 * Order: no atomics.  An image is cut into slices of 8192 pixels of the flat H W array (a function of H W only); a lane adds groups
 * of 8 consecutive pixels, chosen by the pixel index alone; lanes are reduced by wave shuffles, waves through LDS, slices go to the
 * workspace; a second launch of one workgroup sums the slices of each image in slice order and the images in image order.  The
 * result is bit-identical across launches and devices, and for equal values across the three gt types and any alignment of gt.
 * Asynchronous on `stream`, allocates nothing, never synchronises.  Host-side errors, before anything is enqueued: V3D_ERR_BAD_ARG
 * for a null required pointer, one table without the other, a gt_type or valid_mode outside its set, valid_mode 1 without
 * pred_valid, a gt not aligned to its element; V3D_ERR_BAD_SHAPE for a non-positive size, identity tables with hp != H or wp != W,
 * H W >= 2^24 (above it the reference's fp32 counts stop being exact); V3D_ERR_WORKSPACE_TOO_SMALL.
 * v3d_depth_metrics_workspace_bytes returns 0 for a shape the call would reject. */
size_t v3d_depth_metrics_workspace_bytes(int n, int H, int W);
int v3d_depth_metrics_2d(const float* pred, int hp, int wp, const int32_t* row_src, const int32_t* col_src, const void* gt,
                         int gt_type, const uint8_t* pred_valid, int valid_mode, int n, int H, int W, int32_t* counts,
                         double* per_image, double* mean, void* workspace, size_t workspace_bytes, void* stream);

/* Depth supervision of PL3DVNet.forward (csrc/supervision.hip): at each point where mv3d/lightningmodel.py:57-119 supervises a depth
 * map, the masked MAE loss (mv3d/loss.py:6-20) and calc_2d_depth_metrics without a mask, in one pass over the PREDICTION and
 * without a temporary.  ABI version: STILL 9 -- two new symbols, nothing changed.
 *   pred [n, h, w] fp32; gt [n, H, W] fp32 metres; row_src [h], col_src [w] (DEVICE, int32): the row / column of the ground truth
 *   that prediction row r / column c is scored against (the index tables of the nearest resize H -> h, W -> w that the reference
 *   applies to the ground truth; entries are clamped to the ground truth); both NULL = identity, then H == h and W == w.
 * Per pixel (i, r, c): gf = gt[i, row_src[r], col_src[c]], g = double(gf), pf = pred[i, r, c], p = double(pf).
 *   Metrics: the per-pixel rule of v3d_depth_metrics_2d above with valid_mode 0, the same code (csrc/depth2d.h): n_pv, n_m,
 *   S_rel, S_diff, S_inv, S_sqrel, S_sq, c1, c2, c3 with m = g >= 0.5 and g < 65.0, and its deviation (a pixel outside m
 *   contributes nothing).
 *   Loss: where gf != 0.0f (an fp32 comparison; a NaN ground truth is in this mask, as in the reference): n_l += 1 and
 *   S_l += |p - g|, the difference and the sum in float64, every operation rounded on its own.  A non-finite |p - g| is added as it
 *   is and makes the loss non-finite, as the reference's does.  Pixels with 0 < g < 0.5 or g >= 65 count here and not in m.
 * Per image: columns 0-8 of per_image [n, 10] are the nine columns of v3d_depth_metrics_2d (perc_valid is 1), counts [n, 6] are
 *   its five counts and n_l;  per_image[i, 9] = (S_l / double(depth_interval)) / double(float(n_l) + 1e-7f): the reference's
 *   denominator is a float32 tensor and + 1e-7 one fp32 addition; an image without ground truth gives 0.
 *   mean [10] = the float64 sum of the rows of per_image in image order, divided by n; mean[9] is the loss.
 * Order: as v3d_depth_metrics_2d, with slices of 8192 pixels of the flat h w array of the prediction: bit-identical across launches
 * and devices and for any 4-byte alignment of pred and gt.
 * Asynchronous on `stream`, allocates nothing, never synchronises.  Host-side errors, before anything is enqueued: V3D_ERR_BAD_ARG
 * for a null required pointer, one table without the other, pred or gt not aligned to 4 bytes; V3D_ERR_BAD_SHAPE for a
 * non-positive size, identity tables with H != h or W != w, h w >= 2^24; V3D_ERR_WORKSPACE_TOO_SMALL.
 * v3d_depth_supervision_workspace_bytes returns 0 for a shape the call would reject. */
size_t v3d_depth_supervision_workspace_bytes(int n, int h, int w);
int v3d_depth_supervision_f32(const float* pred, int n, int h, int w, const float* gt, int H, int W, const int32_t* row_src,
                              const int32_t* col_src, float depth_interval, int32_t* counts, double* per_image, double* mean,
                              void* workspace, size_t workspace_bytes, void* stream);

/* Exact per-axis order statistics of a 3-D point set (csrc/order_stats.hip): what the volume bounds of a scene take from the
 * back-projected depths (mv3d/eval/processresults.py:324-357: two quantiles per axis), found by radix selection on the fp32 bit
 * patterns without the points ever being stored.  ABI version: STILL 9 -- three new symbols, nothing changed.
 *   v3d_cloud_order_stats_f32        pts [n_pts, 3] fp32 (DEVICE).
 *   v3d_backproject_order_stats_f32  depths [n, h, w] fp32 and proj_inv [n, 16] (DEVICE): the inverse of the 4 x 4 matrix whose
 *                         first three rows are K [R | t], row major; ALL 16 entries are used.  Pixel (i, y, x) with d = depths[i, y,
 *                         x] becomes the point, all fp32, every operation rounded on its own (no fused multiply-add):
 *                           inv = 1 / d
 *                           X_r = ((Pi[r][0] x + Pi[r][1] y) + Pi[r][2]) + Pi[r][3] inv     r = 0..3, left to right, x and y the
 *                                                                                           integer pixel coordinates as floats
 *                           p_a = X_a / X_3                                                 a = 0, 1, 2
 *   A row is dropped if and only if at least one of its three coordinates is a NaN (so d == 0 and d == NaN vanish; rows with an
 *   infinite coordinate stay); it is dropped from all three axes.  N = the rows kept.
 *   Order: k = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000) of the fp32 pattern -- monotone over all non-NaN floats, -inf lowest,
 *   +inf highest, -0.0 just below +0.0.
 *   Ranks, float64, per q = q_host[j] (HOST, n_q of them, read before the call returns): vi = q (N - 1); lo = clamp(floor(vi), 0,
 *   N - 1); hi = min(lo + 1, N - 1).
 *   Outputs (DEVICE): count [1] uint32 = N; stats [n_q, 3, 2] fp32 = per q and axis the lo-th and the hi-th smallest coordinate
 *   (0-based) as the exact bit pattern of an input value.  N == 0: count = 0 and every entry of stats is a NaN.
 *   How: three counting passes over the input (digits of 11 + 11 + 10 key bits), each workgroup counting in LDS and adding its
 *   non-zero bins to the workspace with integer atomics; a one-workgroup kernel between the passes picks each rank's bin.  The
 *   result does not depend on scheduling: repeated launches are bit-identical.  A workgroup's tile is 2048 points.
 * Asynchronous on `stream`, allocates nothing, never synchronises; the workspace (at least v3d_order_stats_workspace_bytes(n_q)
 * bytes, 8-byte aligned) must stay untouched until the work has run.  Host-side errors, before anything is enqueued:
 * V3D_ERR_BAD_ARG for a null pointer, n_q outside 1..4, a q outside [0, 1] (a NaN included), a misaligned workspace;
 * V3D_ERR_BAD_SHAPE for a non-positive size or n h w >= 2^31; V3D_ERR_WORKSPACE_TOO_SMALL.  v3d_order_stats_workspace_bytes returns
 * 0 for an n_q the calls would reject. */
size_t v3d_order_stats_workspace_bytes(int n_q);
int v3d_backproject_order_stats_f32(const float* depths, const float* proj_inv, int n, int h, int w, const double* q_host, int n_q,
                                    uint32_t* count, float* stats, void* workspace, size_t workspace_bytes, void* stream);
int v3d_cloud_order_stats_f32(const float* pts, int n_pts, const double* q_host, int n_q, uint32_t* count, float* stats,
                              void* workspace, size_t workspace_bytes, void* stream);

/* Decoded frames -> the tensors of a scene batch (csrc/frames.hip): the device half of mv3d/dsets/dataset.py:75-91 and :159-219,
 * i.e. crop + cv2.resize(INTER_LINEAR) + the colour normalisation of the colour frames, and the millimetre conversion, the
 * invalid-depth rule, cv2.resize(INTER_NEAREST) and F.interpolate(mode='nearest') of the depth frames, each as one gather through
 * index tables the caller computes (3dvnet_amd/dataset.py: PreprocessImage.linear_tables / nearest_tables, in float64 on the
 * host).  ABI version: STILL 9 -- two new symbols, nothing changed.  Neither call takes scratch memory.
 *
 * v3d_frames_to_images_f32
 *   frames [n, H, W, 3] uint8, interleaved, channel order AS STORED (the reference never swaps OpenCV's BGR and applies mean_rgb[0]
 *   to the first stored channel); y0, y1 [oh] int32 and wy [oh] fp32: the two source rows of output row r and the weight of the
 *   second; x0, x1 [ow] and wx [ow] likewise for columns (all six on the DEVICE; an index outside the frame is clamped to it);
 *   mean_host, std_host: 3 floats each in HOST memory, read before the call returns; images [n, 3, oh, ow] fp32 (the layout
 *   v3d_stem_block_f32 reads).
 *   Per output element (i, ch, r, c), with a, b = frames[i, y0[r], x0[c] | x1[c], ch] and c_, d = the same of row y1[r], converted
 *   to fp32 (exact).  All fp32; every operation below is ONE rounded operation, none of them is fused into a multiply-add, and the
 *   divisions are IEEE divisions:
 *     ux = 1 - wx[c];  top = (a * ux) + (b * wx[c]);  bot = (c_ * ux) + (d * wx[c]);
 *     uy = 1 - wy[r];  v = (top * uy) + (bot * wy[r]);
 *     quantize != 0:  v = rintf(v)      (round half to even: stands in for the uint8 image cv2.resize hands the reference)
 *     x = v / 255.0f;  x = x * 255.0f;  x = x / scale_rgb;  x = x - mean[ch];  images[i, ch, r, c] = x / std[ch]
 *   (that is: three subtractions-from-one, six products and three additions for the blend -- 4 roundings on the path of a value
 *   through each of the two lerps, 8 in all -- and five for the chain.)
 * v3d_frames_to_depths_f32
 *   depth_mm [n, H, W] uint16; ys [oh], xs [ow] int32 (DEVICE): the frame row / column output row r / column c is taken from
 *   (clamped to the frame); depths [n, oh, ow] fp32:  d = float(depth_mm[i, ys[r], xs[c]]) / 1000.0f (IEEE division);
 *   depths[i, r, c] = d > 65.0f ? 0 : d  (dataset.py:160-165; its NaN and inf tests cannot fire on converted integers).
 * Both: asynchronous on `stream`, allocate nothing, never synchronise, every element of the output is written and nothing beside it;
 * repeated launches are bit-identical.  Host-side errors, before anything is enqueued: V3D_ERR_BAD_ARG for a null pointer, a table
 * or output not aligned to 4 bytes (depth_mm: 2), a scale_rgb or std that is zero, a non-finite scale_rgb / mean / std;
 * V3D_ERR_BAD_SHAPE for a non-positive size, 3 n H W >= 2^62 (the kernels index with 64-bit offsets), or an output of 2^31 or more
 * workgroups (256 threads; a thread writes 4 columns x 3 channels of an image, or one depth). */
int v3d_frames_to_images_f32(const uint8_t* frames, int n, int H, int W, const int32_t* y0, const int32_t* y1, const float* wy,
                             const int32_t* x0, const int32_t* x1, const float* wx, int oh, int ow, int quantize, float scale_rgb,
                             const float* mean_host, const float* std_host, float* images, void* stream);
int v3d_frames_to_depths_f32(const uint16_t* depth_mm, int n, int H, int W, const int32_t* ys, const int32_t* xs, int oh, int ow,
                             float* depths, void* stream);

/* Raw scenes -> prepared scene folders, the pixel half (csrc/prepare.hip): the registration of a colour frame into the depth
 * camera (data_preprocess/preprocess_scannet.py:36-70) and the depth-unit conversion of the TUM-format datasets
 * (preprocess_icl_nuim.py:181-185, preprocess_tum_rgbd.py:177-180).  ABI version: STILL 9 -- two new symbols, nothing changed.
 * Neither call takes scratch memory.
 *
 * v3d_register_colour_u8
 *   colour [n, Hc, Wc, 3] uint8, interleaved, channel order AS STORED; homography_host: the nine fp32 entries H00 .. H22 of
 *   K_color K_depth^-1, row major, in HOST memory, read before the call returns (one matrix serves the call: a scene has one pair
 *   of intrinsics); out [n, h, w, 3] uint8.
 *   Per output pixel (i, y, x), x and y the integer pixel coordinates as floats.  All fp32; every operation below is ONE rounded
 *   operation, none of them is fused into a multiply-add, and the divisions are IEEE divisions:
 *     u = ((H00 x) + (H01 y)) + H02;   v = ((H10 x) + (H11 y)) + H12;   d = ((H20 x) + (H21 y)) + H22;
 *     d = d + 1e-8f;   u = u / d;   v = v / d;
 *     gx = (u - Wc / 2) / (Wc / 2);   gy = (v - Hc / 2) / (Hc / 2)        (the reference's normalisers, NOT those of
 *                                     align_corners=True: the sample lands at u (Wc - 1) / Wc.  Kept as the reference has it.)
 *     ix = (gx + 1) * ((Wc - 1) / 2);   iy = (gy + 1) * ((Hc - 1) / 2)    (grid_sample's un-normalisation with align_corners=True,
 *                                     in the form of ATen's CPU kernel; Wc / 2, Hc / 2, (Wc - 1) / 2 and (Hc - 1) / 2 are fp32
 *                                     constants formed once)
 *     jx = rintf(ix);   jy = rintf(iy)                                    (round half to even)
 *     out[i, y, x, :] = colour[i, jy, jx, :] where 0 <= jx < Wc and 0 <= jy < Hc; three zero bytes where (jx, jy) lies outside the
 *     frame or a coordinate is not finite (such a pixel reads nothing).
 *   A thread writes four consecutive pixels of a row: three dword stores where w % 4 == 0 and out is 4-byte aligned, byte stores
 *   otherwise; the two give the same bytes.
 * v3d_lut_u16
 *   out[i] = lut[in[i]] for i < n_elems; in, out [n_elems] uint16, lut [65536] uint16, all on the DEVICE; out must not overlap in.
 *   The depth-unit conversion: the two reference scripts convert in float64 and in float32 and disagree on 144 of the 65 536
 *   inputs, so the caller evaluates the reference's expression in the reference's type once per input value
 *   (3dvnet_amd/preprocess.py: depth_lut) and the kernel holds no arithmetic.  16-byte loads and stores where in and out are
 *   16-byte aligned, element by element otherwise; the two give the same values.
 * Both: asynchronous on `stream`, allocate nothing, never synchronise, every element of the output is written and nothing beside it;
 * the inputs are only read; repeated launches are bit-identical.  Host-side errors, before anything is enqueued: V3D_ERR_BAD_ARG for
 * a null pointer, an in / lut / out of v3d_lut_u16 not aligned to 2 bytes; V3D_ERR_BAD_SHAPE for a non-positive size, 3 n Hc Wc >=
 * 2^62 (the kernels index with 64-bit offsets), or a launch of 2^31 or more workgroups (256 threads; a thread writes 4 pixels, or 8
 * elements of an aligned / 1 of an unaligned v3d_lut_u16). */
int v3d_register_colour_u8(const uint8_t* colour, int n, int Hc, int Wc, const float* homography_host, int h, int w, uint8_t* out,
                           void* stream);
int v3d_lut_u16(const uint16_t* in, size_t n_elems, const uint16_t* lut, uint16_t* out, void* stream);

/* Training, stage 1: backward of v3d_psv_variance_f32 with respect to the features (csrc/psv_backward.hip; the autograd of
 * mvsnet.py:209-216).
 * ABI version: STILL 9 (additive: a new symbol, no changed signature).
 *   Per reference view with cnt edges, per channel and voxel: x_e = bilinear sample of source e (zeros padding: a tap outside
 *   the image adds nothing and receives no gradient), avg = sum_e x_e / cnt, and with gV = grad_var:
 *       g_e = gV * 2 * (x_e - avg) / cnt,     grad_feat[src_e, tap, c] += w_tap * g_e   for the four taps.
 *   Cameras and plane depths are data: the features are the only differentiable input.  The sample positions and weights
 *   are those of the forward kernels, bit for bit (the same device functions, csrc/psv_common.h).
 *   feat_cl      [n_img, Hf, Wf, C]  the features CHANNEL-LAST (the forward takes [n_img, C, Hf, Wf]);  C in {16, 32}
 *   grad_var     [n_ref, C, D, h, w]
 *   grad_feat_cl [n_img, Hf, Wf, C]  out: zero-filled by the call itself, then accumulated -- the caller allocates it
 *                                    uninitialised; an image that appears in no edge ends with exact zeros.
 *   K, R, t, the edge CSR and the scalar geometry arguments are those of v3d_psv_variance_f32.
 * No scratch memory: the call takes none, allocates nothing and never synchronises; asynchronous on `stream`.
 * Contributions are summed with fp32 atomic adds whose arrival order is not fixed: the last bits of the result can differ
 * between two calls with the same inputs (each element stays within the fp32 bound of its sum).
 * Host-side errors: V3D_ERR_BAD_ARG (null pointer), V3D_ERR_UNSUPPORTED (C), V3D_ERR_BAD_SHAPE (a size that is not positive,
 * Hf or Wf > 32759, (Hf + 2) (Wf + 2) >= 2^28 - 1, n_img Hf Wf C >= 2^31, more than 2^31 - 1 workgroups). */
int v3d_psv_variance_backward_f32(const float* feat_cl, const float* K, const float* R, const float* t,
                                  const int32_t* ref_img, const int32_t* edge_ofs, const int32_t* edge_src,
                                  int n_img, int n_ref, int n_edges, int C, int Hf, int Wf, int H, int W,
                                  double depth_start, double depth_interval, int D, int h, int w,
                                  const float* grad_var, float* grad_feat_cl, void* stream);

/* Which warp kernel v3d_psv_variance_* runs for feature maps [n_img, C, Hf, Wf]: 0 the window kernel, 1 the reuse kernel (bordered
 * channel-last copy of 2 GB and more, or the developer option "psv_kernel" = 1), 2 the gather kernel (C = 16, or "psv_kernel" = 2);
 * negative: C or a size the variance rejects.  Only choice 0 writes the layout of v3d_psv_variance_cl8.
 * ABI version: STILL 9 (additive: a new symbol, no changed signature). */
int v3d_psv_kernel_choice(int n_img, int C, int Hf, int Wf);

/* Training, stage 2: backward of v3d_backproject_variance_f32 (csrc/backproject_backward.hip; the autograd of
 * lightningmodel.py:132-174 and :187-235).  The reference builds the sampling grid under torch.no_grad(), so two gradients exist
 * and no other: the variance has none with respect to depth, cameras or offset, and with n_half > 0 the points have none at all.
 * ABI version: STILL 9 (additive: a new symbol, no changed signature).
 *   depth        [n_ref, h, w]; K, R, t, the edge CSR and the scalar arguments are those of v3d_backproject_variance_f32
 *   feat_cl      [n_img, Hf, Wf, C]  the features CHANNEL-LAST (the forward takes [n_img, C, Hf, Wf]);  C in {16, 32}
 *   grad_var     [n_ref*h*w, 2 n_half + 1, C] or NULL          grad_feat_cl [n_img, Hf, Wf, C] out, NULL iff grad_var is NULL
 *   grad_pts     [n_ref*h*w, 1, 3] or NULL, n_half == 0 only   grad_depth   [n_ref, h, w] out, NULL iff grad_pts is NULL
 * Feature gradient.  Per reference view with cnt edges, per pixel, hypothesis and channel: x_e = bilinear sample of source e (zeros
 *   padding), avg = sum_e x_e / cnt, and with gV = grad_var:
 *       g_e = gV * 2 * (x_e - avg) / cnt,     grad_feat[src_e, tap, c] += w_tap * g_e   for the in-image taps.
 *   The call zero-fills grad_feat_cl itself (the caller allocates it uninitialised), then accumulates with fp32 atomic adds whose
 *   arrival order is not fixed: the last bits can differ between two calls with the same inputs (each element stays within the fp32
 *   bound of its sum).  An image that appears in no edge ends with exact zeros.
 * Depth gradient.  pts = R^T (K^-1 (p d) - t), p = (x, y, 1):  grad_depth[r, pix] = sum_j grad_pts[row, j] ray_j, ray = R^T K^-1 p.
 *   One thread per pixel, no atomics: repeated calls are bit-identical.  Evaluation order, dot3_chain(a0, b0, a1, b1, a2, b2) =
 *   fma(a2, b2, fma(a1, b1, a0 * b0)):
 *       c_i   = dot3_chain(Kinv[i,0], x, Kinv[i,1], y, Kinv[i,2], 1)
 *       ray_j = dot3_chain(R[0,j], c_0, R[1,j], c_1, R[2,j], c_2)
 *       g     = dot3_chain(gp_0, ray_0, gp_1, ray_1, gp_2, ray_2)
 *   Kinv is the forward's (fp64 adjugate / determinant, rounded to fp32); x, y are the forward's grid coordinates
 *   (float)(gx * x_step), x_step = (W - 1) / (w - 1) in double, the last column and row pinned to W - 1 and H - 1.
 * Sample positions: the forward's, bit for bit -- hypothesis depth depth + (float)((double)(hyp - n_half) * offset), the same device
 *   functions after it.  A NaN or out-of-range position has no valid tap: it contributes x_e = 0 and receives nothing.
 * No scratch memory: the call takes none, allocates nothing and never synchronises; asynchronous on `stream`.
 * Host-side errors, all before anything is enqueued and before either output is touched: V3D_ERR_BAD_ARG (a null depth, feat_cl,
 *   camera or edge pointer; a grad pair with one side set; neither pair set; grad_pts with n_half > 0), V3D_ERR_UNSUPPORTED (C),
 *   V3D_ERR_BAD_SHAPE (a size that is not positive, H <= 1 or W <= 1, Hf or Wf > 32759, (Hf + 2) (Wf + 2) >= 2^28 - 1,
 *   n_img Hf Wf C >= 2^31, h w >= 2^31, more than 2^31 - 1 workgroups). */
int v3d_backproject_variance_backward_f32(const float* depth, const float* feat_cl, const float* K, const float* R, const float* t,
                                          const int32_t* ref_img, const int32_t* edge_ofs, const int32_t* edge_src,
                                          int n_img, int n_ref, int n_edges, int C, int Hf, int Wf, int H, int W, int h, int w,
                                          double offset, int n_half, const float* grad_var, const float* grad_pts,
                                          float* grad_feat_cl, float* grad_depth, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* V3D_H_ */
