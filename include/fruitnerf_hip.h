/*
 * fruitnerf_hip.h — C ABI of the MI355X-native (gfx950) FruitNeRF ray-marching hot path.
 *
 * The reference (meyerls/FruitNeRF) has no FFI: its hot path is the Nerfstudio Python plugin API
 * (fruit_nerf/fruit_field.py FruitField, fruit_nerf/fruit_nerf.py FruitModel) and the arithmetic
 * runs in nerfstudio==0.3.2 / tiny-cuda-nn.  This header is the C boundary our Python mirror of
 * that API (fruitnerf_amd/) binds with ctypes; every entry point cites the reference interface
 * (file:line relative to /root/reference) whose arithmetic it replaces.  INTEGRATION.md shows the
 * reference-side binding.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless a name ends in _host;
 *   - the caller owns every buffer (parameters, gradients, workspace, outputs);
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*, NULL = default stream);
 *     no entry point synchronises unless documented;
 *   - return value 0 = ok, negative = error (fnr_last_error() gives the message); no exceptions
 *     cross the ABI; nothing falls back to the CPU.
 *   - tensors are dense row-major fp32 unless stated; N = n_rays * S samples, sample n = ray*S + k.
 */
#ifndef FRUITNERF_HIP_H
#define FRUITNERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 13 also covers the per-image camera table (fnr_camera_table, the fnr_*_cams entry points and fnr_camera_rays): pure
 * additions — no existing symbol or struct changed, so a caller built against the earlier 13 runs unchanged.  The TSDF
 * mesh export (fnr_tsdf_volume, the three fnr_tsdf_* entry points) is an addition of the same kind, and so is the mesh
 * connectivity (fnr_mesh_stats, the fnr_mesh_* entry points). */
#define FNR_ABI_VERSION 13
#define FNR_MAX_LEVELS 16
#define FNR_MAX_SEM_LAYERS 4
/* floats in a loss accumulator buffer: per-ray partials are spread over 32 accumulators that sit in 32 different
 * 128-byte lines (atomics to one L2 line serialise at ~12 ns each on MI355X: 4096 rays on one line cost ~35 us);
 * the caller zeroes the buffer and sums all FNR_LOSS_SLOTS floats (see fnr_interlevel_fwd) */
#define FNR_LOSS_SLOTS 1024

enum {
  FNR_OK = 0,
  FNR_ERR_INVALID = -1,     /* bad argument */
  FNR_ERR_UNSUPPORTED = -2, /* configuration not built into this library */
  FNR_ERR_HIP = -3,         /* HIP runtime error (message in fnr_last_error) */
};

/* Multiresolution hash grid, nerfstudio-0.3.2 torch layout: HashEncoding (constructed at
 * fruit_field.py:124-131 and fruit_nerf.py:111-127).  Every level owns T = 2^log2_hashmap_size rows
 * of 2 floats; `scalings` are the integers floor(min_res * growth**level) computed on the HOST in
 * float32 exactly as HashEncoding.__init__ does. */
typedef struct fnr_grid {
  int32_t n_levels;
  int32_t log2_hashmap_size;
  int32_t scalings[FNR_MAX_LEVELS];
  float* table; /* [n_levels << log2_hashmap_size, 2] */
} fnr_grid;

/* RayBundle (nerfstudio.cameras.rays; built at data/fruit_datamanager.py:188-197 and
 * components/ray_generators.py:52-64), after the collider (fruit_nerf.py:161,382-383). */
typedef struct fnr_rays {
  int64_t n_rays;
  const float* origins;          /* [R,3] */
  const float* directions;       /* [R,3] */
  const float* nears;            /* [R]   */
  const float* fars;             /* [R]   */
  const int32_t* camera_indices; /* [R] or NULL */
} fnr_rays;

/* World position -> unit cube (fruit_field.py:168-179).
 * mode 0: SceneContraction(order=inf) then (x+2)/4     (training / rendering)
 * mode 1: SceneBox.get_normalized_positions(x, aabb)   (export: spatial_distortion=None, fruit_nerf.py:183) */
typedef struct fnr_warp {
  int32_t mode;
  float aabb[6]; /* min xyz, max xyz */
} fnr_warp;

/* HashMLPDensityField (fruit_nerf.py:104-129): hash grid -> Linear(2L,H) ReLU Linear(H,1) -> trunc_exp. */
typedef struct fnr_prop_net {
  fnr_grid grid;
  int32_t hidden_dim; /* 16 */
  float* w0;          /* [H, 2L] */
  float* b0;          /* [H] */
  float* w1;          /* [1, H] */
  float* b1;          /* [1] */
} fnr_prop_net;

/* FruitField (fruit_field.py:43-301).  Linear weights are nn.Linear layout [out, in].
 * A second instance of this struct with pointers into the gradient arena describes the gradients.
 * Two shapes are built (everything else returns FNR_ERR_UNSUPPORTED):
 *   `fruit_nerf`                       geo_feat_dim 15, num_layers_semantic 2, hidden_dim_semantics 64
 *   `fruit_nerf_big` / `fruit_nerf_huge` geo_feat_dim 30, num_layers_semantic 3, hidden_dim_semantics 128
 * (fruit_nerf_config.py:27-160; of the widths those configs set only these three reach FruitField,
 * fruit_nerf.py:88-103), both with base / colour width 64, semantic_out_dim 64, appearance 32, 16 hash levels. */
typedef struct fnr_field_net {
  fnr_grid grid;
  int32_t geo_feat_dim;         /* 15 | 30 */
  int32_t hidden_dim;           /* 64 (base MLP width)  */
  int32_t hidden_dim_color;     /* 64 */
  int32_t hidden_dim_semantics; /* 64 | 128 */
  int32_t num_layers_semantic;  /* 2 | 3 */
  int32_t semantic_out_dim;     /* 64 (hidden_dim_transient, fruit_field.py:150) */
  int32_t appearance_dim;       /* 32 */
  int32_t n_images;
  float* base_w0; float* base_b0;           /* [64, 2L], [64] */
  float* base_w1; float* base_b1;           /* [1+geo, 64], [1+geo] */
  float* sem_w[FNR_MAX_SEM_LAYERS];         /* mlp_semantics layers: [64,15],[64,64] | [128,30],[128,128],[64,128] */
  float* sem_b[FNR_MAX_SEM_LAYERS];
  float* head_w; float* head_b;             /* SemanticFieldHead: [1, 64], [1] (components/field_heads.py:29-40) */
  float* col_w[3]; float* col_b[3];         /* mlp_head: [64,16+geo+32],[64,64],[3,64] */
  float* embedding;                         /* embedding_appearance [n_images, 32] */
  int32_t mlp_mode;                         /* FNR_MLP_*: arithmetic of the MLP GEMMs (fnr_field_mlp_fwd / _bwd) */
} fnr_field_net;

/* fnr_field_net.mlp_mode.  The reference trains with mixed_precision=True (fp16 autocast on CUDA,
 * fruit_nerf_config.py:33,69) and runs pure fp32 on the CPU (nerfstudio disables autocast there); parity is judged
 * against the fp32 CPU path.
 *   FNR_MLP_FP32    v_mfma_f32_16x16x4_f32: exact fp32 FMA chains (default; the parity path, 157 TFLOP/s roofline)
 *   FNR_MLP_BF16    v_mfma_f32_16x16x32_bf16 on bf16-rounded operands, fp32 accumulate: throughput mode of BASELINE
 *                   config 2 (2.5 PFLOP/s roofline); outputs differ from fp32 by ~1e-2 relative — NOT parity grade
 *   FNR_MLP_BF16X3  the same instruction on an exact three-way bf16 split of every fp32 operand (6 piece products
 *                   forward, 3 backward): fp32-grade results (~1e-6) at 16/6 resp. 16/3 of the fp32-MFMA rate
 * The bf16 modes are built for the `fruit_nerf` shape; others return FNR_ERR_UNSUPPORTED. */
#define FNR_MLP_FP32 0
#define FNR_MLP_BF16 1
#define FNR_MLP_BF16X3 3

/* ---- library / device ----------------------------------------------------------------------- */
int fnr_abi_version(void);
const char* fnr_last_error(void);
/* Queries the current HIP device; fails loudly when no gfx950 device is present. */
int fnr_device_check(int* cu_count_out, char* name_out, int name_len);

/* Optional HIP-event timing of the entry points (bench.py's roofline leg).  While enabled, every entry
 * point whose op id is set in op_mask brackets what it enqueues with two events recorded on the caller's
 * stream.  fnr_profile_collect synchronises those events and returns up to `capacity` records
 * (op id, units = samples/rays/params the call processed, milliseconds); enable(…) clears old records.
 * Op ids: 0 sample_spaced, 1 weights_pdf, 2 prop_density_fwd, 3 hash_encode_fwd, 4 hash_encode_lattice,
 * 5 field_mlp_fwd, 6 composite_fwd, 7 losses_fwd, 8 interlevel_fwd, 9 distortion, 10 composite_bwd,
 * 11 weights_bwd, 12 field_mlp_bwd, 13 hash_encode_bwd, 14 prop_density_bwd, 15 adam_step, 16 export_compact. */
int fnr_profile_enable(int on, uint64_t op_mask);
/* paused != 0: entry points stop recording events but the records collected so far are kept (bench.py times every
 * tenth step of its timed window: each event pair costs the GPU a ~3 us bubble). */
int fnr_profile_pause(int paused);
int64_t fnr_profile_collect(int32_t* ops_host, int64_t* units_host, float* ms_host, int64_t capacity);
/* Diagnostics of the binned scatter (fnr_hash_encode_bwd*, fnr_prop_density_bwd*): records that did not fit their bin's
 * queue (capacity = 3 x the level's mean) and went to the gradient table through global atomics instead, summed over all
 * calls since the last reset (synchronises the device).  0 in a healthy configuration; such records make the
 * gradient's summation order, hence its last bits, depend on timing.  No counterpart in the reference (torch autograd
 * scatters with atomics throughout). */
int fnr_debug_scatter_overflows(uint64_t* count_host, int reset);
/* records_host[2] = records the accumulate kernels have summed since the last reset: [0] into the field's table
 * (fnr_hash_encode_bwd*), [1] into proposal tables (fnr_prop_density_bwd*) — i.e. the 8 L contributions per sample after
 * run pre-summing.  Each record is 10 bytes written by the emit kernel and read back by the accumulate kernel: the
 * design overhead bench.py reports as roofline.record_queue_bytes.  Synchronises the device.  No counterpart in the
 * reference. */
int fnr_debug_scatter_records(uint64_t* records_host, int reset);

/* ---- caller side: pixel sampling + ray generation --------------------------------------------- */
/* The on-device image batch of a datamanager: uint8 images [M,H,W,3], uint8 fruit masks [M,H,W] (1 = fruit),
 * pinhole cameras (camera-to-world [M,3,4]; fx, fy, cx, cy shared). */
typedef struct fnr_image_set {
  int32_t n_images, H, W;
  const uint8_t* images;
  const uint8_t* masks;
  const float* c2w;
  float fx, fy, cx, cy;
} fnr_image_set;

/* FruitDataManager.next_train (data/fruit_datamanager.py:188-197): PixelSampler (uniform (image, y, x) from
 * u [R,3] in [0,1)) + RayGenerator (pixel centre +0.5, -z forward, unit directions).  train_ids [n_train] maps
 * training slot -> dataset image; camera_indices receives the slot (the appearance-embedding row).
 * c2w_adjusted (optional) [n_train,3,4]: pose-corrected cameras from fnr_camera_adjust, indexed by slot.
 * Outputs: origins/directions [R,3], camera_indices [R], image [R,3] in [0,1], fruit_mask [R] in {0,1}. */
int fnr_sample_pixels(const fnr_image_set* set, const int64_t* train_ids, int n_train, int64_t n_rays, const float* u,
                      const float* c2w_adjusted, float* origins, float* directions, int32_t* camera_indices,
                      float* image, float* fruit_mask, void* stream);

#define FNR_TRAIN_PROLOGUE_MAX_JITTER 5   /* rows of `jitter` one fnr_train_prologue launch draws (level 0 + 4 PDF levels) */
/* The start of a training step in ONE launch (single jitter per ray, the Nerfacto default): draws the step's random
 * numbers itself — Philox4x32-10, counter = (ray, word group, offset), key = seed; the caller advances `offset` by one per
 * step — and performs fnr_camera_adjust (pose_adjustment / c2w_adjusted both set, or both NULL), fnr_sample_pixels and
 * fnr_sample_spaced(level 0, near / far as the collider sets them, one jitter per ray) on them.
 * Outputs besides those of the three entry points: u [R,3] (what fnr_camera_pose_grad needs again) and
 * jitter [n_jitter, R]: row 0 is the jitter level 0 was sampled with, rows 1.. are for the PDF samplers of the following
 * levels.  Given u and jitter, every output is bit-identical to the separate entry points (tests/test_gpu_properties.py). */
int fnr_train_prologue(const fnr_image_set* set, const int64_t* train_ids, int n_train, int64_t n_rays, uint64_t seed,
                       uint64_t offset, const float* pose_adjustment, float* c2w_adjusted, float* u, float* jitter,
                       int n_jitter, float* origins, float* directions, int32_t* camera_indices, float* image,
                       float* fruit_mask, float near_plane, float far_plane, int spacing_kind, int S0,
                       const float* base_bins, float* spacing0, float* euclid0, void* stream);

/* Per-image cameras of a real dataset: what the dataparser reads per dataset or per frame (fl_x, fl_y, cx, cy and the
 * OPENCV coefficients k1..k4, p1, p2; data/fruitnerf_dataparser.py:86-131, 226-273) and hands to
 * Cameras(..., distortion_params=...).  Rows are indexed by DATASET image, like c2w.  The camera-frame direction of pixel
 * (x, y) of image i:  xd = (x + 0.5 - cx_i) / fx_i,  yd = (y + 0.5 - cy_i) / fy_i (OpenCV image coordinates, y down);
 * (xu, yu) = the solution of the OpenCV forward model
 *   r = xu^2 + yu^2,  d = 1 + r (k1 + r (k2 + r (k3 + r k4))),
 *   xd = d xu + 2 p1 xu yu + p2 (r + 2 xu^2),  yd = d yu + 2 p2 xu yu + p1 (r + 2 yu^2)
 * by exactly 10 Newton steps from (xd, yd) (analytic Jacobian, a step is zero where |det| <= 1e-9, no early exit);
 * direction = (xu, -yu, -1).  distortion == NULL or an all-zero row gives the pinhole direction bit for bit. */
typedef struct fnr_camera_table {
  const float* intrinsics;   /* [M,4] fx, fy, cx, cy per DATASET image (indexed like c2w), never NULL */
  const float* distortion;   /* [M,6] k1, k2, k3, k4, p1, p2 (nerfstudio's distortion_params order), or NULL = none */
} fnr_camera_table;

/* fnr_sample_pixels through per-image cameras (the RayGenerator over Cameras with distortion_params that
 * data/fruitnerf_dataparser.py:226-273 builds): set->fx..cy are ignored, H and W stay set-wide. */
int fnr_sample_pixels_cams(const fnr_image_set* set, const fnr_camera_table* cams, const int64_t* train_ids, int n_train,
                           int64_t n_rays, const float* u, const float* c2w_adjusted, float* origins, float* directions,
                           int32_t* camera_indices, float* image, float* fruit_mask, void* stream);
/* fnr_train_prologue through per-image cameras (data/fruit_datamanager.py:188-197 on a real dataset's Cameras): given u
 * and jitter, every output is bit-identical to fnr_camera_adjust + fnr_sample_pixels_cams + fnr_sample_spaced
 * (tests/test_gpu_camera_models.py).  Recorded into step programs like fnr_train_prologue (the table by value). */
int fnr_train_prologue_cams(const fnr_image_set* set, const fnr_camera_table* cams, const int64_t* train_ids, int n_train,
                            int64_t n_rays, uint64_t seed, uint64_t offset, const float* pose_adjustment,
                            float* c2w_adjusted, float* u, float* jitter, int n_jitter, float* origins, float* directions,
                            int32_t* camera_indices, float* image, float* fruit_mask, float near_plane, float far_plane,
                            int spacing_kind, int S0, const float* base_bins, float* spacing0, float* euclid0,
                            void* stream);
/* Full-image rays of ONE camera (Cameras.generate_rays(camera_indices=i), what FruitModel.get_outputs_for_camera_ray_bundle
 * is fed, fruit_nerf.py:382-383): c2w [3,4], intrinsics [4] and distortion [6] (or NULL) are that camera's rows; writes
 * origins / directions [(y1 - y0) W, 3] of the pixel rows [y0, y1), row-major — the same bits fnr_sample_pixels_cams gives
 * for those pixels.  0 <= y0 <= y1 <= H. */
int fnr_camera_rays(const float* c2w, const float* intrinsics, const float* distortion, int H, int W, int y0, int y1,
                    float* origins, float* directions, void* stream);

/* nerfstudio CameraOptimizer(mode="SO3xR3") (fruit_nerf_config.py:39-43): c2w_adjusted[k] =
 * pose_utils.multiply(c2w[train_ids[k]], exp_map_SO3xR3(pose_adjustment[k])), pose_adjustment [n_train,6] =
 * (translation, so3 log-rotation) per training camera. */
int fnr_camera_adjust(const float* c2w, const int64_t* train_ids, int n_train, const float* pose_adjustment,
                      float* c2w_adjusted, void* stream);
/* Backward of fnr_camera_adjust + the ray generation of fnr_sample_pixels: pose_grad [n_train,6] += d(loss)/d(pose)
 * from d_origins / d_directions [R,3] (fnr_position_grad_reduce) of the rays drawn with `u`. */
int fnr_camera_pose_grad(const fnr_image_set* set, const int64_t* train_ids, int n_train, int64_t n_rays,
                         const float* u, const int32_t* camera_indices, const float* pose_adjustment,
                         const float* c2w_adjusted, const float* d_origins, const float* d_directions,
                         float* pose_grad, void* stream);
/* fnr_camera_pose_grad for rays drawn through per-image cameras (fnr_sample_pixels_cams / fnr_train_prologue_cams): the
 * undistorted camera-frame direction is recomputed from u; it does not depend on the pose, nothing more is read. */
int fnr_camera_pose_grad_cams(const fnr_image_set* set, const fnr_camera_table* cams, const int64_t* train_ids,
                              int n_train, int64_t n_rays, const float* u, const int32_t* camera_indices,
                              const float* pose_adjustment, const float* c2w_adjusted, const float* d_origins,
                              const float* d_directions, float* pose_grad, void* stream);

/* The camera optimiser's modes (nerfstudio CameraOptimizerConfig.mode).  The entry points above are FNR_POSE_SO3XR3; the
 * _mode entry points below take `pose_mode` and, where rays are generated, a camera table that may be NULL (= the image
 * set's pinhole, the entry point without _cams); with FNR_POSE_SO3XR3 they give the bits of the entry points above.  Any other pose_mode is an
 * argument error before any launch.
 * FNR_POSE_SE3 (nerfstudio 0.3.2 lie_groups.exp_map_SE3, restated): pose row (v, w), theta = |w| (no clamp), s = theta^2,
 *   R = c I + b_r w w^T + a_r K(w),  t = a_t v + b_t (w x v) + c_t w (w . v),  K(w) = [[0,-wz,wy],[wz,0,-wx],[-wy,wx,0]]
 *   theta >= 1e-2: c = cos theta, a_r = a_t = sin theta / theta, b_r = b_t = (1 - cos theta) / s, c_t = (theta - sin theta) / theta^3
 *   theta <  1e-2: c = 8 / (4 + s) - 1, a_r = c / 2 + 1 / 2, b_r = a_r / 2;  a_t = 1 - s / 6, b_t = 1 / 2 - s / 24, c_t = 1 / 6 - s / 120
 * composed as before: R' = R1 R, t' = t1 + R1 t.  An all-zero row leaves its camera bit for bit and has a finite gradient. */
#define FNR_POSE_SO3XR3 0
#define FNR_POSE_SE3 1
/* fnr_camera_adjust in `pose_mode`.  Not recordable into step programs, like fnr_camera_adjust. */
int fnr_camera_adjust_mode(const float* c2w, const int64_t* train_ids, int n_train, const float* pose_adjustment,
                           int pose_mode, float* c2w_adjusted, void* stream);
/* fnr_train_prologue (cams == NULL) / fnr_train_prologue_cams in `pose_mode`: given u and jitter, every output is
 * bit-identical to fnr_camera_adjust_mode + fnr_sample_pixels[_cams] + fnr_sample_spaced.  Recorded into step programs like
 * fnr_train_prologue (mode and table by value). */
int fnr_train_prologue_mode(const fnr_image_set* set, const fnr_camera_table* cams, int pose_mode, const int64_t* train_ids,
                            int n_train, int64_t n_rays, uint64_t seed, uint64_t offset, const float* pose_adjustment,
                            float* c2w_adjusted, float* u, float* jitter, int n_jitter, float* origins, float* directions,
                            int32_t* camera_indices, float* image, float* fruit_mask, float near_plane, float far_plane,
                            int spacing_kind, int S0, const float* base_bins, float* spacing0, float* euclid0,
                            void* stream);
/* fnr_camera_pose_grad (cams == NULL) / fnr_camera_pose_grad_cams in `pose_mode`: the backward of fnr_camera_adjust_mode +
 * ray generation.  In FNR_POSE_SE3 the translation columns of pose_grad depend on the rotation ones and back.  Not
 * recordable, like fnr_camera_pose_grad. */
int fnr_camera_pose_grad_mode(const fnr_image_set* set, const fnr_camera_table* cams, int pose_mode, const int64_t* train_ids,
                              int n_train, int64_t n_rays, const float* u, const int32_t* camera_indices,
                              const float* pose_adjustment, const float* c2w_adjusted, const float* d_origins,
                              const float* d_directions, float* pose_grad, void* stream);

/* ---- samplers ------------------------------------------------------------------------------- */
/* SpacedSampler.generate_ray_samples (components/ray_samplers.py:54-104; nerfstudio
 * UniformLinDispPiecewiseSampler for the proposal level 0, fruit_nerf.py:151-158).
 * spacing_kind 0: identity (UniformSamplerWithNoise, export); 1: lin/disparity piecewise.
 * base_bins: [S+1] = torch.linspace(0, 1, S+1) evaluated on the HOST (ray_samplers.py:76), so the bins
 *            carry ATen's exact linspace rounding.
 * t_rand: stratified jitter (training mode) or NULL (eval: the bins are base_bins).  t_rand_per_bin = 0: [R], one
 *         number per ray (single_jitter=True: the proposal sampler's level 0); != 0: [R,S+1], one per bin edge
 *         (single_jitter=False, components/ray_samplers.py:79-83 — what the reference's exporter runs, because
 *         FruitModel.setup_inference builds its UniformSamplerWithNoise after eval_setup(), fruit_nerf.py:179-183).
 * Outputs: spacing bins [R,S+1] and euclidean bins [R,S+1]. */
int fnr_sample_spaced(const fnr_rays* rays, int spacing_kind, int S, const float* base_bins, const float* t_rand,
                      int t_rand_per_bin, float* spacing_bins, float* euclid_bins, void* stream);

/* RaySamples.get_weights on the previous level + PDFSampler (nerfstudio; driven from
 * ProposalNetworkSampler, fruit_nerf.py:151-158,318): weights of the S_prev samples, annealed
 * (w^anneal), histogram padding 0.01, inverse-CDF resampling to S_new+1 bins.
 * u_base: [S_new+1] = torch.linspace(0, 1 - 1/(S_new+1), S_new+1) evaluated on the HOST.
 * rand: [R] single-jitter numbers (training) or NULL (eval: centred u).
 * S_new = 0: weights (and median depth) only.
 * median_depth (optional, [R]): DepthRenderer("median") of the S_prev samples (fruit_nerf.py:299-300). */
int fnr_weights_pdf(const fnr_rays* rays, int spacing_kind, int S_prev, int S_new, const float* density,
                    const float* spacing_prev, const float* euclid_prev, float anneal, const float* u_base,
                    const float* rand, float* weights, float* median_depth, float* spacing_new, float* euclid_new, void* stream);

/* ---- use_single_jitter = False: one stratified jitter per bin edge (fruit_nerf.py:149,155 pass the switch to
 * ProposalNetworkSampler; components/ray_samplers.py:79-83: SpacedSampler t_rand [R,S+1], PDFSampler rand [R,S_new+1]) ---
 * THE NUMBERS.  The jitter of edge j of ray r at sampling level l (0 = the spaced sampler, 1.. = the PDF samplers) is
 *   u01(word (j & 3) of Philox4x32-10(counter, key)),
 *   counter = (uint32 r, uint32(r >> 32) ^ ((3 + l) << 24) ^ ((j >> 2) << 8), uint32 offset, uint32(offset >> 32)),
 *   key = (uint32 seed, uint32(seed >> 32)),  u01(x) = (x >> 8) * 2^-24,
 * with seed and offset those of fnr_train_prologue.  Word groups 0 and 1 of the same (seed, offset) are the prologue's and
 * group 2 is fnr_random_background's; levels 0..4 take groups 3..7.  A row has at most FNR_EDGE_JITTER_MAX_EDGES edges (the
 * quad index stays below the group's bits).  Every kernel that consumes these numbers derives them itself. */
#define FNR_EDGE_JITTER_MAX_LEVELS 5
#define FNR_EDGE_JITTER_MAX_EDGES 262144
/* out [n_rays, n_edges] = the numbers above for `level`: what torch.rand((R, S + 1)) is to the reference
 * (components/ray_samplers.py:81-83, PDFSampler's rand likewise), for callers that hand them to fnr_sample_spaced
 * (t_rand_per_bin) / fnr_weights_pdf_edges (rand) or to a comparand.  Recordable like fnr_random_background: a replayed call
 * takes `offset` from fnr_step_scalars.prologue_offset. */
int fnr_edge_jitter(uint64_t seed, uint64_t offset, int level, int64_t n_rays, int n_edges, float* out, void* stream);
/* fnr_train_prologue_mode with one jitter per level-0 bin edge (SpacedSampler with single_jitter=False,
 * components/ray_samplers.py:79-87): the arguments of fnr_train_prologue_mode without jitter / n_jitter.  Given u and
 * fnr_edge_jitter(level 0, S0 + 1 edges), every output is bit-identical to fnr_camera_adjust_mode + fnr_sample_pixels[_cams] +
 * fnr_sample_spaced(t_rand_per_bin = 1); u, rays, pixels and cameras are those of fnr_train_prologue_mode on the same seed
 * and offset.  Recorded into step programs like the other prologues (offset from fnr_step_scalars.prologue_offset). */
int fnr_train_prologue_edges(const fnr_image_set* set, const fnr_camera_table* cams, int pose_mode, const int64_t* train_ids,
                             int n_train, int64_t n_rays, uint64_t seed, uint64_t offset, const float* pose_adjustment,
                             float* c2w_adjusted, float* u, float* origins, float* directions, int32_t* camera_indices,
                             float* image, float* fruit_mask, float near_plane, float far_plane, int spacing_kind, int S0,
                             const float* base_bins, float* spacing0, float* euclid0, void* stream);
/* fnr_weights_pdf with one jitter per new bin edge (PDFSampler with single_jitter=False: rand [R, S_new+1], u = u_base +
 * rand / (S_new+1) per edge).  rand: [R, S_new+1] numbers of the caller, or NULL.  draw != 0 (requires rand == NULL and
 * 1 <= level < FNR_EDGE_JITTER_MAX_LEVELS): the kernel draws fnr_edge_jitter(seed, offset, level) itself — the same bits as
 * rand = that table.  rand == NULL and draw == 0: evaluation (centred u), the bits of fnr_weights_pdf(rand = NULL); seed,
 * offset and level are then ignored.  Everything else is fnr_weights_pdf.  Recorded with fnr_step_scalars.anneal and, for
 * draw != 0, offset from fnr_step_scalars.prologue_offset (the prologue of the same program drew the rays). */
int fnr_weights_pdf_edges(const fnr_rays* rays, int spacing_kind, int S_prev, int S_new, const float* density,
                          const float* spacing_prev, const float* euclid_prev, float anneal, const float* u_base,
                          const float* rand, float* weights, float* median_depth, float* spacing_new, float* euclid_new,
                          uint64_t seed, uint64_t offset, int level, int draw, void* stream);

/* ---- proposal networks ---------------------------------------------------------------------- */
/* HashMLPDensityField.density_fn at the S bin midpoints of every ray (fruit_nerf.py:111-129).
 * feat_save: optional [L][N][2] encoded features kept for fnr_prop_density_bwd. */
int fnr_prop_density_fwd(const fnr_prop_net* net, const fnr_warp* warp, const fnr_rays* rays, const float* euclid_bins,
                         int S, float* density, float* feat_save, void* stream);

/* ---- main field ----------------------------------------------------------------------------- */
/* HashEncoding forward of FruitField.get_density (fruit_field.py:168-186) at the bin midpoints.
 * feats: [L][N][2] (level-major), selector: [N] bytes (the 0<x<1 mask, fruit_field.py:178).
 * jacobian (optional) [L][3][N][2]: d feats / d(unit-cube position), kept for fnr_position_grad_from_jacobian when
 * the rays carry gradients (camera-pose optimisation). */
int fnr_hash_encode_fwd(const fnr_grid* grid, const fnr_warp* warp, const fnr_rays* rays, const float* euclid_bins,
                        int S, float* feats, uint8_t* selector, float* jacobian, void* stream);

/* Same on the orthographic export lattice (data/fruit_datamanager.py:71-121,157-172;
 * components/ray_generators.py:46-66; components/ray_samplers.py:76-94): sample n of the batch is
 * ray (ray_begin + n / n_z), depth index n % n_z, at (xs[ray / n_y], ys[ray % n_y], zs[n % n_z]). */
typedef struct fnr_lattice {
  int32_t n_x, n_y, n_z;
  const float* xs; /* [n_x] torch.linspace values */
  const float* ys; /* [n_y] */
  const float* zs; /* [n_z] sample-midpoint z coordinates */
} fnr_lattice;
int fnr_hash_encode_lattice(const fnr_grid* grid, const fnr_warp* warp, const fnr_lattice* lat, int64_t ray_begin,
                            int64_t n_rays, float* feats, uint8_t* selector, void* stream);

/* mlp_base_mlp + trunc_exp, mlp_semantics + SemanticFieldHead, SHEncoding + mlp_head
 * (fruit_field.py:187-193, 195-232, 234-281) on MFMA.
 * mean_embedding: [32] -> eval/export path (fruit_field.py:217-219,253-256); NULL -> training path,
 * per-ray Embedding[camera_indices] (fruit_field.py:251).
 * h_save [N, fnr_field_h_dim(net)]: the base MLP's raw output (density logit | geo | zero padding to a multiple of
 * 16: 16 floats for geo 15, 32 for geo 30), kept for fnr_field_mlp_bwd.  Optional for the `fruit_nerf` shape; REQUIRED
 * for the `fruit_nerf_big` shape, whose 176 KB of weights do not fit one CU's LDS: it runs as two launches (base +
 * colour, then semantic) that hand h over through this buffer.
 * ray_bias_save (optional) [n_rays,64]: the per-ray part of mlp_head's first layer, kept for fnr_field_mlp_bwd.
 * Outputs per sample: density [N], rgb [N,3], logit [N]; geo_out (optional) [N, geo_feat_dim] = the
 * density embedding `base_mlp_out` returned by get_density (fruit_field.py:187-193).
 * workspace: >= fnr_field_mlp_fwd_workspace_bytes(n_rays) bytes of device scratch: the MFMA fragment image of
 * the weights (packed once per call) and the per-ray part of mlp_head's first layer (SH + appearance
 * embedding are constant along a ray: [n_rays, 64]; with ray_bias_save the workspace only needs
 * fnr_field_mlp_fwd_workspace_bytes(0)).  The image sits at the start of the workspace. */
size_t fnr_field_mlp_fwd_workspace_bytes(int64_t n_rays);
/* Row length of h_save / h_saved for this field shape (16 or 32); -1 if the shape is not built. */
int fnr_field_h_dim(const fnr_field_net* net);
int fnr_field_mlp_fwd(const fnr_field_net* net, const fnr_rays* rays, int S, const float* feats,
                      const uint8_t* selector, const float* mean_embedding, float* density, float* rgb, float* logit,
                      float* geo_out, float* h_save, float* ray_bias_save, void* workspace, size_t workspace_bytes,
                      void* stream);

/* embedding_appearance.mean(dim=0) (fruit_field.py:219,256): out [appearance_dim]. */
int fnr_embedding_mean(const float* embedding, int n_images, int dim, float* out, void* stream);

/* ---- analytic normals (inference side; not recordable: they never run inside a training step) -- */
/* nerfstudio Field.get_normals (fields/base_field.py), for which FruitField.get_density keeps _sample_locations and
 * _density_before_activation (fruit_field.py:180-186): autograd of the density logit h0 = mlp_base(x)[..., 0] with
 * respect to the masked unit-cube sample location, then -F.normalize(gradient, dim=-1).  Per sample, with x [32] the
 * hash features (column 2 l + j):
 *   a1 = W_b0 x + b_b0,  v = 1[a1 > 0] * W_b1[0, :],  df = W_b0^T v,
 *   g[a] = sum_{l,j} jacobian[l][a][n][j] * df[2 l + j],  normal = -g / max(||g||, 1e-12)
 * feats [L][N][2], jacobian [L][3][N][2] and selector [N] are what fnr_hash_encode_fwd wrote for these samples; the
 * gradient is with respect to the location AFTER contraction + (x + 2) / 4, or after the AABB normalisation (what
 * nerfstudio differentiates against): no warp Jacobian enters.  normals [N,3]; gradient (optional) [N,3] receives g.
 * Unselected samples: g = 0, normal = 0.  float32 fmaf chains whatever net->mlp_mode says (one arithmetic: the same
 * bits in every mode and from run to run).  Both built shapes (geo_feat_dim 15 | 30; only the base MLP is read). */
int fnr_field_normals(const fnr_field_net* net, int64_t n_samples, const float* feats, const float* jacobian,
                      const uint8_t* selector, float* normals, float* gradient, void* stream);
/* nerfstudio NormalsRenderer (model_components/renderers.py), as recalled: n = sum_s weights[r][s] * normals[r][s][:]
 * (float32, every product rounded, added one after the other in sample order s = 0 .. S-1), then safe_normalize:
 * n / (||n|| + 1e-10), ||n|| = sqrt((nx nx + ny ny) + nz nz).  shade != 0 additionally applies NormalsShader,
 * (n + 1) / 2 (Nerfacto's outputs["normals"]): a ray of zero weights gives 0, shaded 0.5.
 * weights [R][S] (fnr_composite_fwd's), normals [R][S][3], out [R][3]. */
int fnr_render_normals(int64_t n_rays, int S, const float* weights, const float* normals, int shade, float* out,
                       void* stream);

/* ---- compositing ---------------------------------------------------------------------------- */
/* RaySamples.get_weights + RGBRenderer("last_sample") + AccumulationRenderer + DepthRenderer("median")
 * + SemanticRenderer (fruit_nerf.py:325-348).  training=0 additionally applies nan_to_num / clamp. */
int fnr_composite_fwd(const fnr_rays* rays, int S, const float* euclid_bins, const float* density, const float* rgb,
                      const float* logit, int training, float* weights, float* out_rgb, float* out_accumulation,
                      float* out_depth, float* out_semantics, int64_t* out_label, void* stream);

/* ---- training: losses, backward, optimiser --------------------------------------------------- */
/* get_loss_dict's rgb_loss = MSELoss(image, rgb) and semantics_loss = w * BCEWithLogitsLoss(semantics,
 * fruit_mask) (fruit_nerf.py:171-172,362-366).  losses[0..1] are overwritten with the two scalars and losses[2]
 * with PSNR(rgb, image) = -10 log10(rgb_loss) (get_metrics_dict, fruit_nerf.py:398) — `losses` holds 3 floats;
 * d_rgb [R,3] / d_semantics [R] receive dloss/drgb and dloss/dsemantics (unit upstream). */
int fnr_losses_fwd(int64_t n_rays, const float* rgb, const float* image, const float* semantics,
                   const float* fruit_mask, float semantic_loss_weight, float* losses, float* d_rgb,
                   float* d_semantics, void* stream);

/* nerfstudio interlevel_loss (fruit_nerf.py:368-370) of ONE proposal level against the final level:
 * sum(loss[0..FNR_LOSS_SLOTS)) += mult * mean(clip(w - outer(c, cp, wp), 0)^2 / (w + 1e-7)) — the caller adds the
 * slots up (same-address global atomics serialise at ~12 ns each on MI355X); d_weights_p [R,S_p] = d/d wp. */
int fnr_interlevel_fwd(int64_t n_rays, int S_f, const float* spacing_f, const float* weights_f, int S_p,
                       const float* spacing_p, const float* weights_p, float mult, float* loss, float* d_weights_p,
                       void* stream);

/* nerfstudio distortion_loss on the final level — a metric only (fruit_nerf.py:400):
 * sum(out[0..FNR_LOSS_SLOTS)) += value. */
int fnr_distortion(int64_t n_rays, int S, const float* spacing, const float* weights, float* out, void* stream);

/* use_distortion_loss (Nerfacto's switch; nerfstudio 0.3.2 distortion_loss on the final level): the backward of
 *   loss = mult * mean_r D_r,  D_r = sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 ds_i,
 * m_i / ds_i the midpoint / width of spacing bin i (detached), w the field's compositing weights.  One launch, one wave per ray:
 *   d_weights[k] = (mult / n_rays) g (2 sum_j w_j |m_k - m_j| + (2/3) w_k ds_k),  g = *upstream (device scalar; NULL = 1),
 * the sum taken directly (S terms >= 0); then the backward of RaySamples.get_weights (fnr_weights_bwd's arithmetic) on
 * d_weights, and d_density[k] = d_density[k] + s_k term_k: ONE float32 addition of the value d_density holds (what the
 * compositing backward left there) and the finished term, s_k = 1 or, with gradient_scaling != 0, clamp(m_k^2, 0, 1) of the
 * Euclidean midpoint m_k = (euclid_bins[k] + euclid_bins[k+1]) / 2 as in fnr_composite_options (float32(s_k) x the unscaled
 * term, bit for bit).  spacing, euclid_bins [R,S+1]; density, weights [N]; d_weights [N] out, NULL = not wanted;
 * 1 <= S <= 512; n_rays == 0: nothing to do.  Recordable.  Pure addition at ABI 13. */
int fnr_distortion_bwd(int64_t n_rays, int S, const float* spacing, const float* euclid_bins, const float* density,
                       const float* weights, float mult, const float* upstream, int gradient_scaling, float* d_weights,
                       float* d_density, void* stream);

/* Backward of fnr_composite_fwd (training): g_rgb [R,3], g_semantics [R] -> per-sample d_density [N],
 * d_rgb [N,3], d_logit [N].  Semantic compositing weights are detached (fruit_nerf.py:343-345). */
int fnr_composite_bwd(const fnr_rays* rays, int S, const float* euclid_bins, const float* density, const float* rgb,
                      const float* weights, const float* g_rgb, const float* g_semantics, float* d_density,
                      float* d_rgb, float* d_logit, void* stream);

/* fnr_composite_bwd with the per-ray loss gradients formed in the kernel (ABI 11): g_rgb = 2 (out_rgb - image) / (3 R),
 * g_semantics = semantic_loss_weight (sigmoid(out_semantics) - mask) / R — MSELoss / BCEWithLogitsLoss(mean) backward
 * with unit upstream (fruit_nerf.py:359-367), the expressions fnr_train_losses evaluates, so d_density / d_rgb / d_logit
 * are bit-identical to fnr_train_losses + fnr_composite_bwd.  It makes the backward independent of the losses launch: a
 * training step runs it straight behind the forward and sums the loss values on another stream.
 * out_rgb [R,3], out_semantics [R]: what fnr_composite_fwd returned; image [R,3], mask [R]: the batch. */
int fnr_composite_bwd_targets(const fnr_rays* rays, int S, const float* euclid_bins, const float* density,
                              const float* rgb, const float* weights, const float* out_rgb, const float* image,
                              const float* out_semantics, const float* mask, float semantic_loss_weight,
                              float* d_density, float* d_rgb, float* d_logit, void* stream);
/* fnr_composite_fwd (training = 1) + fnr_composite_bwd_targets as one launch (ABI 13): the same outputs and the same gradients,
 * bit for bit, one kernel boundary less between the field's forward and backward pass of a training step
 * (fruit_nerf.py:325-348 + the autograd of its renderers and of get_loss_dict's rgb / semantic terms, :365-391). */
int fnr_composite_fwd_bwd_targets(const fnr_rays* rays, int S, const float* euclid_bins, const float* density,
                                  const float* rgb, const float* logit, const float* image, const float* mask,
                                  float semantic_loss_weight, float* weights, float* out_rgb, float* out_accumulation,
                                  float* out_depth, float* out_semantics, int64_t* out_label, float* d_density,
                                  float* d_rgb, float* d_logit, void* stream);

/* pass_semantic_gradients = True (FruitNeRF's own switch, fruit_nerf.py:56): SemanticRenderer's weights are NOT detached
 * (fruit_nerf.py:302, 344-345), so the semantic loss reaches the density through the compositing weights:
 * dL/dw_k = g_rgb . (c_k - c_last) + g_semantics * logit_k.  logit [N]: the per-sample logits of fnr_field_mlp_fwd.
 * d_rgb and d_logit are those of the entry points without the suffix, bit for bit; with g_semantics = 0 so is d_density.
 * Pure additions at ABI 13. */
/* fnr_composite_bwd with the semantic term (fruit_nerf.py:344-345).  Not recordable, like fnr_composite_bwd. */
int fnr_composite_bwd_semgrad(const fnr_rays* rays, int S, const float* euclid_bins, const float* density, const float* rgb,
                              const float* logit, const float* weights, const float* g_rgb, const float* g_semantics,
                              float* d_density, float* d_rgb, float* d_logit, void* stream);
/* fnr_composite_bwd_targets with the semantic term (fruit_nerf.py:344-345, 365-391): bit-identical to fnr_train_losses +
 * fnr_composite_bwd_semgrad. */
int fnr_composite_bwd_targets_semgrad(const fnr_rays* rays, int S, const float* euclid_bins, const float* density,
                                      const float* rgb, const float* logit, const float* weights, const float* out_rgb,
                                      const float* image, const float* out_semantics, const float* mask,
                                      float semantic_loss_weight, float* d_density, float* d_rgb, float* d_logit,
                                      void* stream);
/* fnr_composite_fwd_bwd_targets with the semantic term (fruit_nerf.py:325-348 with :344-345 not detached): the arguments
 * of fnr_composite_fwd_bwd_targets; bit-identical to fnr_composite_fwd + fnr_composite_bwd_targets_semgrad. */
int fnr_composite_fwd_bwd_targets_semgrad(const fnr_rays* rays, int S, const float* euclid_bins, const float* density,
                                          const float* rgb, const float* logit, const float* image, const float* mask,
                                          float semantic_loss_weight, float* weights, float* out_rgb,
                                          float* out_accumulation, float* out_depth, float* out_semantics,
                                          int64_t* out_label, float* d_density, float* d_rgb, float* d_logit, void* stream);

/* ---- compositing with Nerfacto's two remaining switches (pure additions at ABI 13) -----------------------------
 * background_color (reference fruit_nerf.py:164; nerfstudio 0.3.2 RGBRenderer.combine_rgb, recalled — DESIGN §2):
 *   out_rgb = sum_k w_k c_k + b (1 - sum_k w_k), b = the last sample's colour ("last_sample", what the entry points above
 *   build) or an explicit triple: "white" (1,1,1), "black" (0,0,0), "random" (U[0,1)^3 per ray and forward pass).  An explicit
 *   b is a constant of the pass: dL/dw_k = g_rgb . (c_k - b), d_rgb_k = g_rgb w_k for EVERY k (no background share on
 *   sample S-1), no nan_to_num of b outside training; the clamp of out_rgb outside training stays.
 * use_gradient_scaling (reference fruit_nerf.py:280-281, 322-323; nerfstudio scale_gradients_by_distance_squared):
 *   forward values unchanged; d_density, d_rgb and d_logit of sample k are multiplied by s_k = clamp(m_k^2, 0, 1),
 *   m_k = (euclid_bins[k] + euclid_bins[k+1]) / 2, in float32, as the LAST operation: each output is float32(s_k) x the
 *   unscaled output, bit for bit.  The proposal levels are not scaled.
 * The options travel in one struct; with {last sample, no scaling} every entry point below makes the launch of its
 * counterpart above (same kernel, same bits). */
#define FNR_BACKGROUND_LAST_SAMPLE 0
#define FNR_BACKGROUND_EXPLICIT 1
typedef struct fnr_composite_options {
  int32_t background;          /* FNR_BACKGROUND_* */
  int32_t background_stride;   /* explicit: floats between the rows of background_rgb — 3: one triple per ray [R,3];
                                * 0: one triple for every ray */
  const float* background_rgb; /* explicit: device; ignored (may be NULL) for the last sample */
  int32_t gradient_scaling;    /* != 0: use_gradient_scaling */
  int32_t semantic_gradients;  /* != 0: pass_semantic_gradients (the `_semgrad` entry points) */
} fnr_composite_options;
/* fnr_composite_fwd; recordable. */
int fnr_composite_fwd_opt(const fnr_rays* rays, int S, const float* euclid_bins, const float* density, const float* rgb,
                          const float* logit, int training, const fnr_composite_options* options, float* weights,
                          float* out_rgb, float* out_accumulation, float* out_depth, float* out_semantics,
                          int64_t* out_label, void* stream);
/* fnr_composite_bwd / fnr_composite_bwd_semgrad (logit [N]: read with semantic_gradients only); not recordable. */
int fnr_composite_bwd_opt(const fnr_rays* rays, int S, const float* euclid_bins, const float* density, const float* rgb,
                          const float* logit, const float* weights, const float* g_rgb, const float* g_semantics,
                          const fnr_composite_options* options, float* d_density, float* d_rgb, float* d_logit,
                          void* stream);
/* fnr_composite_bwd_targets(_semgrad): bit-identical to fnr_train_losses + fnr_composite_bwd_opt; recordable. */
int fnr_composite_bwd_targets_opt(const fnr_rays* rays, int S, const float* euclid_bins, const float* density,
                                  const float* rgb, const float* logit, const float* weights, const float* out_rgb,
                                  const float* image, const float* out_semantics, const float* mask,
                                  float semantic_loss_weight, const fnr_composite_options* options, float* d_density,
                                  float* d_rgb, float* d_logit, void* stream);
/* fnr_composite_fwd_bwd_targets(_semgrad): bit-identical to fnr_composite_fwd_opt (training) +
 * fnr_composite_bwd_targets_opt; recordable. */
int fnr_composite_fwd_bwd_targets_opt(const fnr_rays* rays, int S, const float* euclid_bins, const float* density,
                                      const float* rgb, const float* logit, const float* image, const float* mask,
                                      float semantic_loss_weight, const fnr_composite_options* options, float* weights,
                                      float* out_rgb, float* out_accumulation, float* out_depth, float* out_semantics,
                                      int64_t* out_label, float* d_density, float* d_rgb, float* d_logit, void* stream);
/* background_color = "random": out [n_rays,3] = U[0,1)^3 per ray from the generator of fnr_train_prologue — Philox4x32-10,
 * counter (ray, word group 2, offset), key seed, words 0-2 through (x >> 8) * 2^-24; the prologue's own numbers are word
 * groups 0 and 1 of the same (seed, offset).  Recordable: a replayed call takes `offset` from
 * fnr_step_scalars.prologue_offset, like the prologue. */
int fnr_random_background(uint64_t seed, uint64_t offset, int64_t n_rays, float* out, void* stream);

/* Backward of RaySamples.get_weights for a proposal level: d_weights [R,S] (x *upstream if non-NULL, a
 * device scalar) -> d_density [R,S]. */
int fnr_weights_bwd(int64_t n_rays, int S, const float* euclid_bins, const float* density, const float* weights,
                    const float* d_weights, const float* upstream, float* d_density, void* stream);

/* Backward of fnr_field_mlp_fwd (training path): accumulates (+=) the Linear weight/bias/embedding gradients
 * into `grads` and writes dL/dfeatures d_feats [L][N][2] for fnr_hash_encode_bwd.
 * workspace: >= fnr_field_mlp_bwd_workspace_bytes(n_rays, S) bytes. */
size_t fnr_field_mlp_bwd_workspace_bytes(int64_t n_rays, int S);
int fnr_field_mlp_bwd(const fnr_field_net* net, const fnr_field_net* grads, const fnr_rays* rays, int S,
                      const float* feats, const float* h_saved, const float* ray_bias_saved /* optional */,
                      const float* packed_saved /* optional: the start of fnr_field_mlp_fwd's workspace (its fragment
                      image), valid if the weights have not changed since */,
                      const uint8_t* selector, const float* d_density,
                      const float* d_rgb, const float* d_logit, float* d_feats, void* workspace, size_t workspace_bytes,
                      void* stream);

/* fnr_field_mlp_bwd + the input gradient of the hash grid for rays that carry gradients (camera-pose optimisation,
 * fruit_nerf_config.py:39-43; the reference's positions are forced requires_grad, fruit_field.py:180-182):
 * jacobian [L][3][N][2] = what fnr_hash_encode_fwd saved (d feats / d unit-cube position), d_position [N][4] receives
 * dL/d(unit-cube position) of every sample (xyz, w = 0) — the contraction of d_feats with the Jacobian, formed by the
 * base-branch kernel from the dL/dfeats it holds in registers (bf16-pipe modes; one extra launch in fp32 mode).
 * fnr_position_grad_reduce(n_levels = 1, partial = d_position) finishes dL/d(origins, directions). */
int fnr_field_mlp_bwd_rays(const fnr_field_net* net, const fnr_field_net* grads, const fnr_rays* rays, int S,
                           const float* feats, const float* h_saved, const float* ray_bias_saved /* optional */,
                           const float* packed_saved /* optional */, const uint8_t* selector, const float* d_density,
                           const float* d_rgb, const float* d_logit, float* d_feats, const float* jacobian,
                           float* d_position, void* workspace, size_t workspace_bytes, void* stream);

/* fnr_field_mlp_bwd (+ optionally the input gradient, as fnr_field_mlp_bwd_rays: jacobian and d_position both NULL or
 * both set) with the optimiser step of every parameter this backward produces the gradient of — the Linear weights and
 * biases of mlp_base_mlp / mlp_semantics / field_head_semantics / mlp_head and the appearance embedding, i.e. the
 * "fields" group without the hash table (fruit_nerf_config.py:51-56) — fused in (single-process training).  The thread
 * that owns a gradient entry (k_reduce_dw, k_embedding_grad: fixed-order sums, single writer) applies torch.optim.Adam /
 * RAdam to that parameter and leaves the gradient entry ZERO.  grad_arena: base of the gradient buffer `grads` points
 * into; weight_adam->params / exp_avg / exp_avg_sq: bases of the buffers that parallel it element for element (the
 * caller's flat arenas).  Bit-identical to fnr_field_mlp_bwd followed by fnr_adam_step / fnr_radam_step(zero_grad = 1)
 * on those spans (tests/test_gpu_training_parity.py). */
int fnr_field_mlp_bwd_adam(const fnr_field_net* net, const fnr_field_net* grads, const fnr_rays* rays, int S,
                           const float* feats, const float* h_saved, const float* ray_bias_saved /* optional */,
                           const float* packed_saved /* optional */, const uint8_t* selector, const float* d_density,
                           const float* d_rgb, const float* d_logit, float* d_feats, const float* jacobian /* optional */,
                           float* d_position /* optional */, const struct fnr_table_adam* weight_adam,
                           const float* grad_arena, void* workspace, size_t workspace_bytes, void* stream);

/* The MLP backward under pass_semantic_gradients = True (fruit_nerf.py:56): the geometry feature that feeds mlp_semantics
 * is NOT detached (fruit_field.py:202-203, 263-264), so the input gradient of mlp_semantics' first layer joins dL/dh
 * between the colour and the base branch: d_feats, the weight gradients of mlp_base_mlp, d_position and everything behind
 * them see the semantic loss; the gradients of mlp_semantics, the head, mlp_head and the embedding are those of
 * fnr_field_mlp_bwd, bit for bit.  One entry point for the three forms of the parent: jacobian / d_position both NULL
 * (fnr_field_mlp_bwd) or both set (fnr_field_mlp_bwd_rays); weight_adam / grad_arena both NULL or both set
 * (fnr_field_mlp_bwd_adam, the Adam slot patched on replay in the same way).  Recordable when weight_adam is set. */
int fnr_field_mlp_bwd_semgrad(const fnr_field_net* net, const fnr_field_net* grads, const fnr_rays* rays, int S,
                              const float* feats, const float* h_saved, const float* ray_bias_saved /* optional */,
                              const float* packed_saved /* optional */, const uint8_t* selector, const float* d_density,
                              const float* d_rgb, const float* d_logit, float* d_feats, const float* jacobian /* optional */,
                              float* d_position /* optional */, const struct fnr_table_adam* weight_adam /* optional */,
                              const float* grad_arena /* optional */, void* workspace, size_t workspace_bytes, void* stream);


/* Backward of fnr_hash_encode_fwd: adds (+=) the trilinear scatter of d_feats [L][N][2] into
 * grid_grad->table for the levels [level_begin, level_begin + level_count) (all levels: 0, n_levels; data-parallel
 * training calls it per group of levels so that a group's rows can be all-reduced while the next group is being
 * scattered).  Binned through per-bin queues in `workspace` (>= fnr_hash_scatter_workspace_bytes(n_samples,
 * level_count, log2_hashmap_size)) because global fp32 atomics top out at ~21 G/s on MI355X (hash_scatter.hip).
 * workspace_clean: 0 = the library zeroes the queue counters first (any buffer); 1 = the caller passes a buffer whose
 * last use was a completed call of the same entry point with the same sizes — the kernels leave the counters zeroed,
 * which saves one memset launch per call. */
size_t fnr_hash_scatter_workspace_bytes(int64_t n_samples, int n_levels, int log2_hashmap_size);
int fnr_hash_encode_bwd(const fnr_grid* grid_grad, const fnr_warp* warp, const fnr_rays* rays,
                        const float* euclid_bins, int S, const float* d_feats, int level_begin, int level_count,
                        void* workspace, size_t workspace_bytes, int workspace_clean, void* stream);

/* fnr_hash_encode_bwd over ALL levels with the optimiser step of the table ("fields" group, fruit_nerf_config.py:51-56)
 * fused in (single-process training: with
 * several ranks the gradient has to exist for the all-reduce).  The workgroup that owns a bin of rows holds their summed
 * gradient in LDS and applies torch.optim.Adam (algorithm 0) / RAdam (1) to those rows — parameters, exp_avg and
 * exp_avg_sq are the TABLE's slices [n_levels << log2_hashmap_size, 2] of the caller's arenas, `step` is the
 * optimiser's step count of this update (>= 1), grad_scale / weight_decay as in fnr_adam_step.  The gradient table
 * (grid_grad->table) is left as it was (zero): it is only read where an overflowed queue spilled into it.  Results are
 * bit-identical to fnr_hash_encode_bwd followed by fnr_adam_step / fnr_radam_step on the table's span.
 * touched (optional, table entry points only; weight_decay must be 0): persistent bitmap owned by the caller, one bit per
 * PAIR of table rows (4 floats; bit i of word i / 32, index relative to `params`), zeroed when the moments are zero: "some
 * row of this pair has ever received a gradient".  A pair whose bit is clear and which receives no gradient now has
 * exp_avg = exp_avg_sq = 0, so torch's update of it is exactly zero (m = v = 0 stay, p - lr / bc1 * (0 / eps) = p) and
 * its 24 B per parameter are neither read nor written ("sparse-touch skipping"): every level is hashed,
 * so the coarse levels only ever use (res + 1)^3 of their 2^T rows — 27 % of the `fruit_nerf` table never moves.  The
 * kernel sets the bits of the pairs it touches.  NULL: every row is swept.  Results are bit-identical either way. */
typedef struct fnr_table_adam {
  int32_t algorithm;
  float lr, beta1, beta2, eps;
  int32_t slot; /* step programs (below): 1..FNR_PROGRAM_ADAM_SLOTS = on replay `lr` and `step` come from
                   fnr_step_scalars.adam[slot - 1]; 0 = the recorded values.  Ignored outside a replay. */
  int64_t step;
  float grad_scale, weight_decay;
  float* params;
  float* exp_avg;
  float* exp_avg_sq;
  uint32_t* touched;
} fnr_table_adam;
int fnr_hash_encode_bwd_adam(const fnr_grid* grid_grad, const fnr_warp* warp, const fnr_rays* rays,
                             const float* euclid_bins, int S, const float* d_feats, void* workspace,
                             size_t workspace_bytes, int workspace_clean, const fnr_table_adam* adam, void* stream);

/* fnr_camera_pose_grad with the pose table's optimiser step (camera_optimizer group, fruit_nerf_config.py:39-43) fused in
 * (single-process training): adam->params is
 * pose_adjustment [n_train,6] (read for the gradient, then updated), exp_avg / exp_avg_sq its moments; pose_grad is
 * added to the new gradient and left ZERO.  Bit-identical to fnr_camera_pose_grad followed by fnr_adam_step /
 * fnr_radam_step(zero_grad = 1) over the 6 n_train floats. */
int fnr_camera_pose_grad_adam(const fnr_image_set* set, const int64_t* train_ids, int n_train, int64_t n_rays,
                              const float* u, const int32_t* camera_indices, const float* c2w_adjusted,
                              const float* d_origins, const float* d_directions, float* pose_grad,
                              const fnr_table_adam* adam, void* stream);
/* fnr_camera_pose_grad_adam for rays drawn through per-image cameras (camera_optimizer group, fruit_nerf_config.py:39-43,
 * on a dataset with per-frame intrinsics / distortion): bit-identical to fnr_camera_pose_grad_cams followed by the
 * optimiser step; recorded into step programs like fnr_camera_pose_grad_adam (the table by value, the Adam slot patched). */
int fnr_camera_pose_grad_adam_cams(const fnr_image_set* set, const fnr_camera_table* cams, const int64_t* train_ids,
                                   int n_train, int64_t n_rays, const float* u, const int32_t* camera_indices,
                                   const float* c2w_adjusted, const float* d_origins, const float* d_directions,
                                   float* pose_grad, const fnr_table_adam* adam, void* stream);
/* fnr_camera_pose_grad_adam (cams == NULL) / fnr_camera_pose_grad_adam_cams in `pose_mode` (FNR_POSE_SO3XR3 | FNR_POSE_SE3):
 * bit-identical to fnr_camera_pose_grad_mode followed by the optimiser step; recorded into step programs like
 * fnr_camera_pose_grad_adam (mode and table by value, the Adam slot patched). */
int fnr_camera_pose_grad_adam_mode(const fnr_image_set* set, const fnr_camera_table* cams, int pose_mode,
                                   const int64_t* train_ids, int n_train, int64_t n_rays, const float* u,
                                   const int32_t* camera_indices, const float* c2w_adjusted, const float* d_origins,
                                   const float* d_directions, float* pose_grad, const fnr_table_adam* adam, void* stream);

/* Backward of fnr_prop_density_fwd: d_density [R,S] -> += into grads (table, w0, b0, w1, b1).
 * d_position (optional) [N,4]: gradient w.r.t. each sample's unit-cube position (xyz, w = 0) for
 * fnr_position_grad_reduce(n_levels = 1) — only needed when the rays carry gradients (camera-pose optimiser).
 * workspace >= fnr_prop_density_bwd_workspace_bytes(N, L, log2_hashmap_size).  (prop_bwd.hip: these four entry points
 * compose the same launches; the table's part goes through the binned scatter of hash_scatter.hip.) */
size_t fnr_prop_density_bwd_workspace_bytes(int64_t n_samples, int n_levels, int log2_hashmap_size);
int fnr_prop_density_bwd(const fnr_prop_net* net, const fnr_prop_net* grads, const fnr_warp* warp,
                         const fnr_rays* rays, const float* euclid_bins, int S, const float* feat_save,
                         const float* d_density, float* d_position, void* workspace, size_t workspace_bytes,
                         int workspace_clean, void* stream);

/* fnr_prop_density_bwd with the optimiser step of THIS network's parameters fused in (single-process training; a network
 * that serves one proposal level — with use_same_proposal_network the levels' gradients have to be summed first):
 * table_adam = the hash table's slices of the caller's arenas (as in fnr_hash_encode_bwd_adam: the scatter's accumulate
 * kernel steps the rows it owns, the gradient table stays zero), weight_adam / grad_arena = the arenas' bases (as in
 * fnr_field_mlp_bwd_adam: k_prop_reduce steps w0 / b0 / w1 / b1 and leaves their gradient entries zero).  Bit-identical to
 * fnr_prop_density_bwd followed by fnr_adam_step / fnr_radam_step(zero_grad = 1) on the network's spans. */
int fnr_prop_density_bwd_adam(const fnr_prop_net* net, const fnr_prop_net* grads, const fnr_warp* warp,
                              const fnr_rays* rays, const float* euclid_bins, int S, const float* feat_save,
                              const float* d_density, float* d_position, const fnr_table_adam* table_adam,
                              const fnr_table_adam* weight_adam, const float* grad_arena, void* workspace,
                              size_t workspace_bytes, int workspace_clean, void* stream);

/* Both proposal levels of a training step through ONE entry point (arrays of two: network, gradients, warp, bins, S,
 * saved features, d_density, d_position, workspace, ...; the same rays): each level's MLP backward, weight reduction and
 * scatter emit as in fnr_prop_density_bwd, then ONE accumulate launch over both levels' bins (each level has 160
 * workgroups of 64 KiB LDS on 256 CUs: side by side they cost the longer of the two).  The two levels need their own
 * network, gradients and workspace.  table_adam [2] + weight_adam + grad_arena: all NULL, or all set for the fused
 * optimiser steps of fnr_prop_density_bwd_adam.  Results are those of the two separate calls, bit for bit. */
int fnr_prop_density_bwd_pair(const fnr_prop_net* const* nets, const fnr_prop_net* const* grads,
                              const fnr_warp* const* warps, const fnr_rays* rays, const float* const* euclid_bins,
                              const int* S, const float* const* feat_save, const float* const* d_density,
                              float* const* d_position, const fnr_table_adam* const* table_adam,
                              const fnr_table_adam* weight_adam, const float* grad_arena, void* const* workspace,
                              const size_t* workspace_bytes, const int* workspace_clean, void* stream);
/* fnr_prop_density_bwd_pair with its launches in two groups: both levels' MLP backward + weight reduction first — after
 * them d_position[0] and [1] are final, and position_ready_event (a hipEvent_t created by the caller; optional) is
 * recorded on `stream` — then both levels' emit launches and the joint accumulate (~210 us for `fruit_nerf`).  A caller
 * with a second stream finishes the ray gradients and takes the camera optimiser's step next to that scatter instead
 * of behind it.  Same launches on the same inputs: results are those of fnr_prop_density_bwd_pair, bit for bit. */
int fnr_prop_density_bwd_pair_split(const fnr_prop_net* const* nets, const fnr_prop_net* const* grads,
                                    const fnr_warp* const* warps, const fnr_rays* rays, const float* const* euclid_bins,
                                    const int* S, const float* const* feat_save, const float* const* d_density,
                                    float* const* d_position, const fnr_table_adam* const* table_adam,
                                    const fnr_table_adam* weight_adam, const float* grad_arena, void* const* workspace,
                                    const size_t* workspace_bytes, const int* workspace_clean, void* stream,
                                    void* position_ready_event);

/* All of get_loss_dict / get_metrics_dict (fruit_nerf.py:359-372, 396-401: rgb_loss, semantics_loss, interlevel_loss; psnr, distortion) for one training batch in ONE launch:
 * fnr_losses_fwd + fnr_interlevel_fwd for
 * each of the n_levels (<= FNR_MAX_PROPOSAL_LEVELS) proposal levels against the final level + (want_distortion)
 * fnr_distortion, and the sum of the accumulator slots.  losses [5] = rgb_loss, semantics_loss, psnr,
 * interlevel_loss, distortion (0 when not wanted); d_rgb [R,3], d_semantics [R] (both NULL: not written — a caller whose
 * composite backward forms them itself, fnr_composite_bwd_targets), d_weights_p[l] [R,S_p[l]] as the single calls give them.  accum: FNR_TRAIN_LOSSES_ACCUM_FLOATS floats (loss slots + completion counters), zeroed by
 * the caller before its FIRST use; every completed call leaves it zeroed again (the last workgroup cleans up), so a caller
 * that keeps the buffer launches no fill per step — after a FAILED call the caller must zero it again.  The slots hold
 * 64-bit fixed point (2^-34 resolution): a contribution that is not finite or beyond its row's bound (4096 for the per-ray
 * interlevel / distortion terms, 2^28 / waves for the per-wave squared-error and BCE sums) makes every loss of the call
 * NaN instead of wrapping the sum.
 * S_p / spacing_p / weights_p / d_weights_p are host arrays of n_levels entries.
 * d_density_p (optional, with euclid_p [R,S_p+1] and density_p [R,S_p]): level l's d(loss)/d(density) [R,S_p[l]] =
 * fnr_weights_bwd of that level with d_weights_p[l] as upstream, computed in the same pass (bit-identical); then
 * d_weights_p / d_weights_p[l] may be NULL. */
#define FNR_MAX_PROPOSAL_LEVELS 4
#define FNR_TRAIN_LOSSES_ACCUM_FLOATS (4 * FNR_LOSS_SLOTS + 33 * 32)
int fnr_train_losses(int64_t n_rays, const float* rgb, const float* image, const float* semantics,
                     const float* fruit_mask, float semantic_loss_weight, float* d_rgb, float* d_semantics, int S_f,
                     const float* spacing_f, const float* weights_f, int n_levels, const int* S_p,
                     const float* const* spacing_p, const float* const* weights_p, float* const* d_weights_p,
                     const float* const* euclid_p, const float* const* density_p, float* const* d_density_p,
                     float interlevel_mult, int want_distortion, float* accum, float* losses, void* stream);

/* ---- gradient of the rays (camera-pose optimisation, fruit_nerf_config.py:39-43) ----------------- */
/* Input gradient of fnr_hash_encode_fwd: partial [L][N][4] = per level d(loss)/d(unit-cube position) of every
 * sample, from d_feats [L][N][2] and the PARAMETER table (autograd of HashEncoding w.r.t. its input through the
 * trilinear offsets; `positions * selector` zeroes it outside the unit cube, fruit_field.py:178-179). */
int fnr_hash_encode_input_grad(const fnr_grid* grid, const fnr_warp* warp, const fnr_rays* rays,
                               const float* euclid_bins, int S, const float* d_feats, float* partial, void* stream);
/* Sums `partial` [n_levels][N][4] over the levels, applies the transposed Jacobian of the position warp
 * (SceneContraction + (x+2)/4, or AABB normalisation) and of Frustums.get_positions (p = o + d (t0+t1)/2, bins
 * detached), and ADDS the per-ray sums to d_origins [R,3] and d_directions [R,3]. */
int fnr_position_grad_reduce(const fnr_warp* warp, const fnr_rays* rays, const float* euclid_bins, int S,
                             int n_levels, const float* partial, float* d_origins, float* d_directions,
                             void* stream);
/* fnr_position_grad_reduce over up to FNR_MAX_POSITION_SOURCES sources in one launch: source q contributes the ray
 * gradient carried by partials[q] ([n_levels[q]][N_q][4], N_q = n_rays * S[q]) through warps[q] and the frustum chain of
 * euclid_bins[q] ([n_rays, S[q] + 1]).  accumulate = 0: d_origins / d_directions are WRITTEN (no zero fill needed);
 * 1: added to.  The per-source sums are those of fnr_position_grad_reduce, added in source order. */
#define FNR_MAX_POSITION_SOURCES 4
int fnr_position_grad_reduce_multi(int n_sources, const fnr_warp* const* warps, const fnr_rays* rays,
                                   const float* const* euclid_bins, const int* S, const int* n_levels,
                                   const float* const* partials, int accumulate, float* d_origins, float* d_directions,
                                   void* stream);

/* Same result from the Jacobian fnr_hash_encode_fwd saved: d_origins / d_directions [R,3] += the ray gradient of
 * d_feats [L][N][2] (no table gathers in the backward pass). */
int fnr_position_grad_from_jacobian(const fnr_warp* warp, const fnr_rays* rays, const float* euclid_bins, int S,
                                    int n_levels, const float* jacobian, const float* d_feats, float* d_origins,
                                    float* d_directions, void* stream);

/* torch.optim.Adam step (no amsgrad; fruit_nerf_config.py:47-56) over a flat arena of n floats (n % 4 == 0); the
 * gradient is multiplied by grad_scale first (1/world_size after an all-reduce(SUM)), weight_decay is torch's L2 form
 * (grad += weight_decay * param; 0 for the model's groups, 1e-2 for the camera optimiser, fruit_nerf_config.py:41),
 * and the gradient is zeroed afterwards when zero_grad != 0.  `step` is the 1-based step count for the bias
 * corrections. */
int fnr_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                  float beta2, float eps, int64_t step, float grad_scale, float weight_decay, int zero_grad,
                  void* stream);
/* torch.optim.RAdam step with the same conventions (RAdamOptimizerConfig of fruit_nerf_big / fruit_nerf_huge,
 * fruit_nerf_config.py:77-80,97-106,125-160): rectified adaptive update once rho_t > 5, plain bias-corrected momentum
 * before. */
int fnr_radam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                   float beta2, float eps, int64_t step, float grad_scale, float weight_decay, int zero_grad,
                   void* stream);

/* The optimisers of a method's parameter groups (fruit_nerf_config.py:47-56, 97-106, 148-160: one torch.optim instance and
 * scheduler per group) as ONE launch over several spans of one arena (the groups differ in learning rate and step count;
 * each is a few thousand to a few million floats and a launch of its own cost more than its traffic).  Span k updates
 * elements [offset, offset + count) (both multiples of 4) exactly as fnr_adam_step (algorithm 0) / fnr_radam_step (1)
 * with its own lr / step would.  n_spans <= FNR_MAX_ADAM_SPANS; `spans` is host memory. */
#define FNR_MAX_ADAM_SPANS 8
typedef struct fnr_adam_span {
  int64_t offset, count;
  int64_t step;
  float lr;
  int32_t reserved;
} fnr_adam_span;
int fnr_adam_step_spans(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int n_spans,
                        const fnr_adam_span* spans, int algorithm, float beta1, float beta2, float eps,
                        float grad_scale, float weight_decay, int zero_grad, void* stream);

/* fnr_adam_step_spans for an optimiser that a torch.amp.GradScaler drives (torch.optim's `_step_supports_amp_scaling`
 * protocol): what that scaler decides per step, and the spans' step counts, stay in DEVICE memory — the call contains no
 * stream synchronisation and no copy to the host.  Per element the arithmetic of fnr_adam_step_spans, in the same order.
 *   spans       host memory, n_spans <= FNR_MAX_ADAM_SPANS; offset / count multiples of 4, lr per span (schedulers run on
 *               the host); the `step` field is ignored.
 *   steps       device, int64 [n_spans], in/out: optimiser steps span k has actually TAKEN.  Advanced by 1 iff the step
 *               is not skipped; the bias corrections (and RAdam's rho_t / rectification, "not rectified" for
 *               rho_t <= 5) are computed on the device from the post-increment count in double and rounded to float
 *               where fnr_adam_step_spans rounds them.
 *   grad_scale  device float or NULL (= 1): every gradient is multiplied by (float)(1.0 / (double)*grad_scale), the
 *               factor of GradScaler.unscale_.
 *   found_inf   device float or NULL (= 0): when *found_inf != 0 parameters, moments and counters stay untouched bit for
 *               bit; with zero_grad != 0 the gradient spans are zeroed all the same.
 *   scalars     device, FNR_ADAM_DEV_SCALAR_FLOATS floats of scratch owned by the caller, consumed in stream order: calls
 *               that share a block must be enqueued on one stream.
 * Two launches: a one-workgroup prologue (thread k owns counter k: reads the flags and its counter, writes the span's
 * scalars to `scalars`, bumps the counter), then the sweep, which reads `scalars` and never a counter.  All argument
 * checks run on the host before the first launch. */
#define FNR_ADAM_DEV_SCALAR_FLOATS 32
int fnr_adam_step_spans_dev(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int n_spans,
                            const fnr_adam_span* spans, int64_t* steps, int algorithm, float beta1, float beta2,
                            float eps, const float* grad_scale, const float* found_inf, float weight_decay,
                            int zero_grad, float* scalars, void* stream);

/* ---- step programs: a training step's launch sequence, recorded once and replayed natively (ABI 12) ------------- */
/* The reference's loop is nerfstudio's Python Trainer (fruit_pipeline.py:120-146 under Trainer.train_iteration); ours
 * (fruitnerf_amd/training.py::TrainingSteps) is ~30 calls of this ABI per step on two HIP streams.  Every pointer of a
 * step is stable (parameter arenas, persistent workspaces, the caller's double-buffered step arena), so the sequence is
 * recorded ONCE per step shape and replayed by one call: between fnr_program_begin and fnr_program_end the recordable
 * entry points called on this thread — fnr_train_prologue, fnr_prop_density_fwd, fnr_weights_pdf, fnr_hash_encode_fwd,
 * fnr_field_mlp_fwd, fnr_composite_fwd, fnr_train_losses, fnr_composite_bwd_targets, fnr_field_mlp_bwd_adam,
 * fnr_composite_bwd_targets_semgrad, fnr_composite_fwd_bwd_targets_semgrad, fnr_field_mlp_bwd_semgrad (with weight_adam),
 * fnr_composite_fwd_opt, fnr_composite_bwd_targets_opt, fnr_composite_fwd_bwd_targets_opt, fnr_random_background,
 * fnr_edge_jitter, fnr_train_prologue_edges, fnr_weights_pdf_edges,
 * fnr_hash_encode_bwd_adam, fnr_prop_density_bwd_pair(_split), fnr_position_grad_reduce_multi,
 * fnr_camera_pose_grad_adam and the stream operations below — run as usual AND append themselves (arguments by value,
 * host structs / host arrays copied) to the program; any other entry point that enqueues device work poisons the
 * recording (fnr_program_end then fails and the program stays empty).  fnr_program_replay calls them again in order, on
 * the streams they were recorded on, with the per-step scalars patched in.  The caller keeps every recorded buffer
 * alive and unchanged in place for as long as it replays the program. */
#define FNR_PROGRAM_ADAM_SLOTS 4
typedef struct fnr_step_scalars {
  uint64_t prologue_offset; /* fnr_train_prologue(_edges), fnr_random_background, fnr_edge_jitter, fnr_weights_pdf_edges(draw): `offset` (the step's random-number counter) */
  float anneal;             /* fnr_weights_pdf: `anneal` */
  int32_t reserved;
  struct {
    float lr;
    int32_t reserved;
    int64_t step;           /* 0 = keep the recorded lr / step of this slot */
  } adam[FNR_PROGRAM_ADAM_SLOTS]; /* by fnr_table_adam.slot - 1 */
  float* losses;            /* fnr_train_losses: `losses` (5 floats, device); NULL = the recorded buffer */
} fnr_step_scalars;
typedef struct fnr_program fnr_program;
int fnr_program_create(fnr_program** out);
int fnr_program_destroy(fnr_program* program);
/* begin: the program is emptied and this thread records into it; end: stops recording, fails (and empties the program)
 * if an unrecordable entry point ran in between; abort: stops recording and empties the program. */
int fnr_program_begin(fnr_program* program);
int fnr_program_end(fnr_program* program);
int fnr_program_abort(fnr_program* program);
int64_t fnr_program_size(const fnr_program* program);
/* name of the entry point behind operation i (a static string), NULL when out of range */
const char* fnr_program_op_name(const fnr_program* program, int64_t i);
/* scalars NULL: every operation with its recorded arguments.  Stops at the first failing operation and returns its code. */
int fnr_program_replay(const fnr_program* program, const fnr_step_scalars* scalars);
/* Stream dependencies (recordable): events are hipEvent_t created with timing disabled, owned by the caller.
 * fnr_stream_wait_stream: work enqueued on `waiting` after the call runs after everything enqueued on `signalling`
 * before it (one event of an internal pool is recorded and waited for; the host does not block). */
int fnr_event_create(void** event_out);
int fnr_event_destroy(void* event);
int fnr_event_record(void* event, void* stream);
int fnr_stream_wait_event(void* stream, void* event);
int fnr_stream_wait_stream(void* waiting, void* signalling);

/* ---- export --------------------------------------------------------------------------------- */
/* sample_volume's masks + gathers (export/exporter_utils.py:111-153) as an order-preserving stream
 * compaction.  Sets: 0 = semantic_colormap (sigmoid(logit) > 0.9 and density >= 70),
 * 1 = semantic (logit >= 3 and density >= 70), 2 = density (density >= 70).
 * points[s]: [capacity,3] world positions (fruit_nerf.py:259), colors[s]: [capacity,4] = rgb || sigmoid(x)
 * with x = logit (sets 0,1) or density (set 2).  counts: uint64[3] running totals (device), advanced by
 * this call; entries beyond `capacity` are counted but not written.
 * Sample positions come either from the lattice (lat != NULL: rays [ray_begin, ray_begin+n_rays) x n_z) or
 * from an explicit array positions[n_positions,3] (lat == NULL; outputs['point_location'], fruit_nerf.py:259).
 * workspace: >= fnr_export_workspace_bytes(n_samples) bytes. */
size_t fnr_export_workspace_bytes(int64_t n_samples);
int fnr_export_compact(const fnr_lattice* lat, int64_t ray_begin, int64_t n_rays, const float* positions,
                       int64_t n_positions, const float* density,
                       const float* rgb, const float* logit, float* const points[3], float* const colors[3],
                       int64_t capacity, uint64_t* counts, void* workspace, void* stream);
/* Nerfstudio's generate_point_cloud, one batch: point = origins + directions * depth (fp32, the product and the sum
 * rounded separately, like torch); kept when every coordinate lies strictly inside (box_min, box_max) — HOST pointers to
 * 3 floats, both NULL: everything is kept.  Kept points and their rgb are appended in ray order to points / colors
 * [capacity][3] at the running total *count (device uint64), which this call advances; entries beyond `capacity` are
 * counted but not written.  workspace: >= fnr_export_workspace_bytes(n_rays) bytes. */
int fnr_depth_points(const float* origins, const float* directions, const float* depth, const float* rgb,
                     int64_t n_rays, const float* box_min, const float* box_max, float* points, float* colors,
                     int64_t capacity, uint64_t* count, void* workspace, void* stream);
/* fnr_depth_points with one more per-ray attribute, normals [n_rays][3] (generate_point_cloud with
 * normal_method="model_output": the rendered normal of a ray belongs to its point): appended to normals_out
 * [capacity][3] under the same mask, in the same order and at the same running count.  points, colors and *count are
 * bit-identical to fnr_depth_points on the same input. */
int fnr_depth_points_normals(const float* origins, const float* directions, const float* depth, const float* rgb,
                             const float* normals, int64_t n_rays, const float* box_min, const float* box_max,
                             float* points, float* colors, float* normals_out, int64_t capacity, uint64_t* count,
                             void* workspace, void* stream);

/* ---- TSDF mesh export: depth fusion + marching tetrahedra (csrc/tsdf.hip) ----------------------- */
/* What Nerfstudio's `ns-export tsdf` computes (exporter/tsdf_utils.py, as recalled — Nerfstudio is not available to this
 * project, so THIS text is the contract; tests/tsdf_reference.py restates it in float64).  Pure additions to ABI 13.
 *
 * Volume.  dims = (nx, ny, nz) NODES over the axis-aligned box [lo, hi]; voxel_size = (hi - lo) / dims per axis (fp32);
 * node (i, j, k) sits at lo + (i, j, k) * voxel_size and has the linear index (i * ny + j) * nz + k (z fastest).
 * values / weights: [nx][ny][nz], colors: [nx][ny][nz][3], fp32; the caller initialises values = -1, weights = 0,
 * colors = 0.  truncation = truncation_margin * voxel_size.x (Nerfstudio's margin: 5).  2 <= every dim <= 2048. */
typedef struct fnr_tsdf_volume {
  int32_t dims[3];
  float lo[3];
  float hi[3];
  float truncation_margin;
  float max_weight; /* >= 1.  1: Nerfstudio's clamp (the last valid camera wins); large: the plain running average */
  float* values;
  float* weights;
  float* colors;
} fnr_tsdf_volume;
#define FNR_TSDF_DEPTH_Z 0   /* depth images hold z, the distance along the optical axis (what Nerfstudio compares) */
#define FNR_TSDF_DEPTH_RAY 1 /* depth images hold the distance along the pixel's ray (this model's "depth" output) */
/* Fuses n_cameras pinhole cameras, in the order given, into the volume.  c2w: [n][3][4] camera-to-world rows (R | t),
 * intrinsics: [n][4] = fx, fy, cx, cy, depth: [n][H][W], rgb: [n][H][W][3], mask: [n][H][W] bytes or NULL (all valid);
 * all DEVICE arrays.  For node p and camera c, every operation in fp32:
 *   q = R^T (p - t)  (Nerfstudio's camera frame: x right, y up, -z forward),  z = -q.z;
 *   u = fx * q.x / z + cx,  v = fy * (-q.y) / z + cy   (pinhole; distortion is not modelled);
 *   col = rint(u - 0.5), row = rint(v - 0.5), ties to even (grid_sample(mode="nearest", align_corners=False));
 *   a pixel outside the image or with mask byte 0 reads depth 0;
 *   voxel_depth = z (FNR_TSDF_DEPTH_Z) or |q| (FNR_TSDF_DEPTH_RAY);  dist = sampled depth - voxel_depth;
 *   the sample is valid iff z > 0 && sampled depth > 0 && dist > -truncation; for a valid sample
 *     s = clamp(dist / truncation, -1, 1),  value = (value * w + s) / (w + 1), each colour channel likewise with the
 *     sampled rgb,  w = min(w + 1, max_weight).
 * One thread per node; the camera loop runs inside the kernel, so a node's five floats are read and written once per call
 * and the result is bit-identical however the cameras are split into calls.  n_cameras == 0 launches nothing. */
int fnr_tsdf_integrate(const fnr_tsdf_volume* volume, int32_t n_cameras, const float* c2w, const float* intrinsics,
                       int32_t H, int32_t W, const float* depth, const float* rgb, const uint8_t* mask,
                       int32_t depth_kind, void* stream);
/* Surface extraction: marching tetrahedra on the cells of the node grid.  A node is inside iff value < 0 (unobserved
 * nodes, -1, are inside).  Cell (i, j, k) has the corners (i + dx, j + dy, k + dz), corner id = dx + 2 dy + 4 dz, and is
 * split into six tetrahedra around its main diagonal: tetrahedron t walks from corner 0 to corner 7 along the axes in the
 * order t = 0: x y z, 1: x z y, 2: y x z, 3: y z x, 4: z x y, 5: z y x, its corners c0..c3 being the four corners on that
 * walk.  The same split in every cell, so faces match across cells.
 *   Edges.  Every tetrahedron edge runs from a node a to the node b = a + (dx, dy, dz) with direction code
 * m = dx + 2 dy + 4 dz in 1..7 (three axes, three face diagonals, the body diagonal); its key is 8 * index(a) + m.  It is
 * active iff its endpoints differ in side, and carries one vertex, shared by every cell around it:
 *   t = (0 - v_a) / (v_b - v_a);  position = p_a + t * (p_b - p_a), from a, the endpoint with the smaller index;
 *   colour = colour of the nearer endpoint: of a iff |v_a| <= |v_b| (a tie goes to the smaller index);
 *   normal = normalise(g_a + t * (g_b - g_a)), g = the central-difference gradient of values in world units (one-sided
 *   at the border); a zero vector stays zero.
 *   Faces.  With the inside corners i0 < i1 .. and the outside corners o0 < o1 .. of a tetrahedron (positions on its walk):
 *   one inside: (i0 o0, i0 o1, i0 o2); three inside: (o0 i0, o0 i1, o0 i2); two inside: the quad (i0 o0, i0 o1, i1 o1,
 *   i1 o0) as the triangles (A, B, C), (A, C, D); each triangle then wound so that its normal points towards the outside
 *   (positive values).  The 16-case table is derived at compile time from these rules (csrc/tsdf.hip).
 *   Order.  Vertices ascend by edge key; faces ascend by (cell index = index of its corner 0, t, triangle).  Both come
 * from exclusive scans: the arrays are a function of the volume alone, whatever the launch geometry.
 * fnr_tsdf_mesh_count writes counts[2] (DEVICE uint64) = number of vertices, number of faces, and leaves the scan
 * results in `workspace` (>= FNR_TSDF_MESH_WORKSPACE_BYTES(nx * ny * nz) bytes, 8-byte aligned).  The caller reads the
 * counts (a synchronisation), allocates, and calls fnr_tsdf_mesh_emit with the SAME workspace and the unchanged volume:
 * vertices / normals / colors [n_vertices][3] fp32 (world units), faces [n_faces][3] int32; entries beyond n_vertices /
 * n_faces are not written.  More than 2^31 - 1 vertices cannot be indexed and are refused. */
#define FNR_TSDF_MESH_WORKSPACE_BYTES(n_nodes) (4 * (size_t)(n_nodes) + 16 * (((size_t)(n_nodes) + 255) / 256) + 16)
int fnr_tsdf_mesh_count(const fnr_tsdf_volume* volume, uint64_t* counts, void* workspace, size_t workspace_bytes,
                        void* stream);
int fnr_tsdf_mesh_emit(const fnr_tsdf_volume* volume, const void* workspace, size_t workspace_bytes, int64_t n_vertices,
                       int64_t n_faces, float* vertices, float* normals, float* colors, int32_t* faces, void* stream);

/* ---- triangle-mesh connectivity: components, their statistics, selection (csrc/mesh.hip) ------- */
/* What users of a TSDF mesh do next with Open3D — cluster_connected_triangles(), remove_triangles_by_mask(),
 * select_by_index() — as recalled; Open3D is not available to this project, so THIS text is the contract
 * (tests/mesh_components_reference.py restates it in float64).  Pure additions to ABI 13.
 *
 * Mesh.  vertices [V][3] fp32, faces [F][3] int32 with indices in [0, V); V, F <= 2^31 - 1; DEVICE arrays.  F == 0 is
 * valid everywhere and launches nothing.  An index outside [0, V) is found on the device and refused (see Errors).
 *
 * Connectivity.  Two faces are connected iff they share an undirected edge {a, b} with a != b; sharing only a vertex does
 * not connect them.  Each face contributes three edge incidences, one per slot s (the edge from index s to index
 * (s + 1) % 3); a slot with a == b (a face that repeats an index) contributes nothing: no incidence, no connection.  An
 * edge with three or more incidences connects all its faces; a face listed twice connects to itself and to its copy.  A
 * component is numbered by the rank of its smallest face index among all components' smallest face indices: component 0
 * holds face 0 — the order a sweep from face 0 upwards assigns.  fnr_mesh_components writes face_component [F] int32 and
 * counts[0] (DEVICE uint64) = the number of components, and leaves the edge table in `workspace` (>=
 * fnr_mesh_workspace_bytes(n_faces) bytes, 16-byte aligned) for fnr_mesh_component_stats.  No vertex array is read: edge
 * keys are 64 bits, (min(a, b) << 32) | max(a, b), so V may be 2^31 - 1 whatever F is.
 *   How.  An open-addressing table of at least 4 F slots (key, smallest face of the edge, incidence count), slots claimed
 * by 64-bit compare-and-swap at device scope; union-find over faces in which every face of an edge is united with the
 * edge's smallest face and a hook always puts the larger root under the smaller, so a component's root is its smallest
 * face; the trees are flattened in a later launch (the launch boundary is the visibility guarantee) and the roots numbered
 * by an exclusive scan over "is a root".  No workgroup waits for another; the only retry loops are compare-and-swap
 * retries; every probe sequence is bounded by the table size and every parent chain by F.
 *
 * Statistics of component c, over its faces in the mesh (fnr_mesh_component_stats, arrays of n_components entries):
 *   exact integers: n_faces; boundary_edges — edges with exactly one incidence; nonmanifold_edges — edges with three or
 *   more (an edge belongs to the component of its faces; all faces of an edge are in one component by construction);
 *   exact fp32: lo[3], hi[3] over the vertices the component's faces reference;
 *   float64 raw sums, the vertices converted to float64 first, every operation rounded (no fused multiply-add):
 *     area   = sum |(v1 - v0) x (v2 - v0)| / 2,
 *     volume = sum v0 . (v1 x v2) / 6   — signed: positive for outward normals, and meaningful only where
 *              boundary_edges == nonmanifold_edges == 0,
 *     moment[3] = sum area_f * (v0 + v1 + v2) / 3   (the surface centroid is moment / area; the caller divides).
 *   Orientation consistency is NOT checked: a closed component whose faces disagree in winding has a meaningless volume.
 *   The float64 sums are the same bits for the same mesh, run to run: no floating-point atomics; the faces are grouped by
 *   component with a stable radix sort (count -> scan -> ordered emit per 8-bit digit, so a component's faces ascend) and
 *   added by a fixed-shape segmented reduction — runs of one component inside blocks of 256 sorted positions in position
 *   order, a component's block records by lane l = l, l + 64, ... in order, the 64 lanes by a butterfly.
 *   The call needs the workspace fnr_mesh_components left for these faces and its n_components; it reads the workspace's
 *   header back first (a synchronisation) and refuses an n_components that is inconsistent with counts.
 *
 * Selection.  Given face_keep [F] uint8, the new mesh keeps the faces with a non-zero byte in their old order and the
 * vertices those faces reference in their old order.  fnr_mesh_select_count writes counts[2] (DEVICE uint64) = number of
 * kept vertices, number of kept faces, and leaves both index maps in `workspace` (>= fnr_mesh_select_workspace_bytes
 * bytes, 16-byte aligned); the caller reads the counts, allocates, and calls fnr_mesh_select_emit with the SAME workspace
 * and faces: new_faces [F'][3] re-indexed, vertex_ids [V'] ascending old vertex indices, face_ids [F'] ascending old face
 * indices (the caller gathers positions and attributes with vertex_ids).  Entries beyond the given sizes are not written.
 *
 * Errors.  Arguments are checked on the host before anything is launched.  A bad index or label and any exceeded bound set
 * an error word in the workspace; every entry point here that launches reads it back before it returns (a
 * synchronisation of `stream`) and then fails with FNR_ERR_INVALID and a message in fnr_last_error. */
typedef struct fnr_mesh_stats {
  int32_t* n_faces;           /* [C] */
  int32_t* boundary_edges;    /* [C] */
  int32_t* nonmanifold_edges; /* [C] */
  float* lo;                  /* [C][3] */
  float* hi;                  /* [C][3] */
  double* area;               /* [C] */
  double* volume;             /* [C] */
  double* moment;             /* [C][3] */
} fnr_mesh_stats;
size_t fnr_mesh_workspace_bytes(int64_t n_faces);
int fnr_mesh_components(int64_t n_vertices, int64_t n_faces, const int32_t* faces, int32_t* face_component,
                        uint64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int fnr_mesh_component_stats(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                             const int32_t* face_component, int64_t n_components, void* workspace,
                             size_t workspace_bytes, const fnr_mesh_stats* out, void* stream);
size_t fnr_mesh_select_workspace_bytes(int64_t n_vertices, int64_t n_faces);
int fnr_mesh_select_count(int64_t n_vertices, int64_t n_faces, const int32_t* faces, const uint8_t* face_keep,
                          uint64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int fnr_mesh_select_emit(int64_t n_vertices, int64_t n_faces, const int32_t* faces, const void* workspace,
                         size_t workspace_bytes, int64_t n_new_vertices, int64_t n_new_faces, int32_t* new_faces,
                         int32_t* vertex_ids, int32_t* face_ids, void* stream);

/* ---- triangle-mesh filters: vertex rows, smoothing, normals, vertex clustering (csrc/mesh_filters.hip) ---- */
/* What users of a mesh do with Open3D before they look at connectivity and sizes — filter_smooth_laplacian(),
 * filter_smooth_taubin(), compute_vertex_normals(), simplify_vertex_clustering() — as recalled; Open3D is not available to
 * this project, so THIS text is the contract (tests/mesh_filters_reference.py restates it in float64, and the device
 * arrays equal the restatement's bit for bit).  Pure additions to ABI 13.  The mesh, the error word and the host-side
 * argument checks are those of the connectivity section; V == 0 and F == 0 are valid everywhere and launch no kernel.
 *
 * The primitive is the per-vertex ROW with a fixed order: offsets int32 [V + 1] (offsets[0] = 0, ascending, offsets[V] =
 * E) and entries int32 [E]; row a is entries[offsets[a] .. offsets[a + 1]).  Every floating-point sum below is the
 * sequential float64 sum of a row's terms in row order, starting from 0.0, every product, difference, quotient and square
 * root rounded once (no fused multiply-add, no floating-point atomics): a result has one defined bit pattern.
 *
 * Vertex rows (fnr_mesh_vertex_rows_count / _emit; 6 n_faces <= 2^31 - 1).  No vertex array is read.
 *   kind = FNR_MESH_ROWS_NEIGHBOURS: row a holds every b != a that shares a face with a, each once, ascending.  A face
 *     that repeats an index still connects its distinct indices; the rows are symmetric, and they are the same arrays
 *     for any order of the faces.
 *   kind = FNR_MESH_ROWS_FACES: row a holds every face that lists a, each once, ascending.
 *   _count writes counts[0] (DEVICE uint64) = E and leaves the sorted keys in `workspace` (>=
 *   fnr_mesh_vertex_rows_workspace_bytes bytes, 16-byte aligned); the caller reads E, allocates, and calls _emit with the
 *   SAME workspace, sizes and kind: offsets [V + 1], entries [E].
 *   How.  One 64-bit key (row << 32) | entry per ordered pair of a face's slots (NEIGHBOURS, six a face) or per slot
 *   (FACES, three a face); a stable least-significant-digit radix sort (count -> one-workgroup scan -> ordered emit per
 *   8-bit digit) over only the bytes V and F need; the first copy of every key with row != entry is marked, the marks are
 *   scanned, and offsets[r] is the scan at the first sorted key of a row >= r (a bounded binary search).
 *
 * Smoothing (fnr_mesh_smooth; rows of kind NEIGHBOURS).  Positions are converted to float64 once, kept in float64 across
 * the n_steps steps (two buffers in `workspace`, >= fnr_mesh_smooth_workspace_bytes bytes; one launch per step) and rounded
 * to fp32 once at the end.  Step s, for a vertex p with a non-empty row, over its neighbours n in row order:
 *     w_n = 1 (FNR_MESH_WEIGHTS_UNIFORM) or 1 / (sqrt((dx*dx + dy*dy) + dz*dz) + 1e-12), d = p - p_n
 *           (FNR_MESH_WEIGHTS_INVERSE_DISTANCE);
 *     S += w_n * p_n per axis, W += w_n;   p' = p + factors[s] * (S / W - p).
 * A vertex with an empty row keeps its position.  factors is a HOST array of n_steps doubles: Laplacian smoothing is
 * [lambda] * n, Taubin smoothing [lambda, mu] * n (mu < -lambda < 0).  n_steps == 0 copies the positions.  out may not
 * alias vertices.
 *
 * Vertex normals (fnr_mesh_vertex_normals; rows of kind FACES).  The face term is (v1 - v0) x (v2 - v0) in float64, not
 * normalised (area weighting); the vertex sum n runs over the row in row order; normals = n / sqrt((nx*nx + ny*ny) +
 * nz*nz) rounded to fp32, and (0, 0, 0) where that square is not positive.  workspace: >= 64 bytes.
 *
 * Vertex clustering (fnr_mesh_cluster_count / _emit).  voxel_size is a positive double, origin a HOST pointer to three
 * finite doubles.  The cell of a vertex per axis is floor((double(v) - origin) / voxel_size); a non-finite coordinate, a
 * negative cell and a cell >= 2^21 are refused.  (Open3D's simplify_vertex_clustering puts the origin at the minimum
 * bound minus half a voxel; the caller does.)  A cluster is the set of ALL vertices of one cell, referenced or not;
 * clusters are numbered by the rank of their smallest member among all clusters' smallest members: cluster 0 holds
 * vertex 0.  _count writes vertex_cluster [V] and counts[2] (DEVICE uint64) = number of clusters V', number of kept faces
 * F', and leaves its tables in `workspace` (>= fnr_mesh_cluster_workspace_bytes bytes); _emit, with the SAME workspace,
 * sizes and faces, writes the cluster rows — offsets [V' + 1], members [V] ascending inside a cluster — and new_faces
 * [F'][3] with face_ids [F']: the faces re-indexed by cluster, in their old order and with their old rotation, without
 *   - a face with two equal new indices, and
 *   - a later duplicate of a kept face: two faces are duplicates iff their new triples are equal after rotating each to
 *     start at its smallest index.  The same triangle with the opposite winding is therefore NOT a duplicate.
 *   How.  Vertices sorted by cell key (the same stable sort, so a cell's vertices ascend and its first is its smallest),
 *   runs numbered by a scan; faces sorted by their rotated triple (equal triples ascend by face), the first of a run kept.
 *
 * Row mean (fnr_mesh_rows_mean): out[r] = float64 sum of values[m] [3] over row r's members m in row order, divided by the
 * member count, rounded to fp32; (0, 0, 0) for an empty row.  values is fp32 [n_values][3].  workspace: >= 64 bytes.  The
 * clustered positions, colours and normals are row means over the cluster rows.
 *
 * Errors.  As in the connectivity section; besides a bad face index, rows that are not rows (offsets that do not ascend
 * within [0, n_entries], an entry outside its array) and a vertex outside the cells are found on the device and refused. */
#define FNR_MESH_ROWS_NEIGHBOURS 0
#define FNR_MESH_ROWS_FACES 1
#define FNR_MESH_WEIGHTS_UNIFORM 0
#define FNR_MESH_WEIGHTS_INVERSE_DISTANCE 1
size_t fnr_mesh_vertex_rows_workspace_bytes(int64_t n_vertices, int64_t n_faces, int32_t kind);
int fnr_mesh_vertex_rows_count(int64_t n_vertices, int64_t n_faces, const int32_t* faces, int32_t kind, uint64_t* counts,
                               void* workspace, size_t workspace_bytes, void* stream);
int fnr_mesh_vertex_rows_emit(int64_t n_vertices, int64_t n_faces, int32_t kind, const void* workspace,
                              size_t workspace_bytes, int64_t n_entries, int32_t* offsets, int32_t* entries, void* stream);
size_t fnr_mesh_smooth_workspace_bytes(int64_t n_vertices);
int fnr_mesh_smooth(int64_t n_vertices, const float* vertices, int64_t n_entries, const int32_t* offsets,
                    const int32_t* neighbours, int32_t n_steps, const double* factors, int32_t weights, float* out,
                    void* workspace, size_t workspace_bytes, void* stream);
int fnr_mesh_vertex_normals(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                            int64_t n_entries, const int32_t* offsets, const int32_t* face_rows, float* normals,
                            void* workspace, size_t workspace_bytes, void* stream);
size_t fnr_mesh_cluster_workspace_bytes(int64_t n_vertices, int64_t n_faces);
int fnr_mesh_cluster_count(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                           double voxel_size, const double* origin, int32_t* vertex_cluster, uint64_t* counts,
                           void* workspace, size_t workspace_bytes, void* stream);
int fnr_mesh_cluster_emit(int64_t n_vertices, int64_t n_faces, const int32_t* faces, void* workspace,
                          size_t workspace_bytes, int64_t n_clusters, int64_t n_new_faces, int32_t* offsets,
                          int32_t* members, int32_t* new_faces, int32_t* face_ids, void* stream);
int fnr_mesh_rows_mean(int64_t n_rows, int64_t n_entries, const int32_t* offsets, const int32_t* members,
                       int64_t n_values, const float* values, float* out, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---- point-cloud front-end of the counting stage ---------------------------------------------- */
/* FruitClustering.cluster (clustering/clustering_base.py:183-207) runs, on the exported cloud, Open3D's
 * remove_radius_outlier (:141-143), Open3D's voxel_down_sample (:138-139) and sklearn.cluster.DBSCAN (:199-200).
 * These three entry points replace those library calls; clouds are [n][3] float64 device arrays (Open3D / PLY
 * precision), every integer result (counts, labels) is bit-exact with the CPU libraries.  lo/hi/min_bound/max_bound
 * are HOST pointers to 3 doubles: the axis-aligned bounds of the cloud (Open3D's GetMinBound/GetMaxBound).
 * workspace: >= fnr_cloud_workspace_bytes(n) bytes, caller-owned, contents undefined afterwards. */
size_t fnr_cloud_workspace_bytes(int64_t n_points);
/* lo_hi[6] (device) = min x, y, z, max x, y, z of the cloud (n >= 1); workspace >= 64 bytes. */
int fnr_cloud_bounds(const double* xyz, int64_t n, double* lo_hi, void* workspace, size_t workspace_bytes,
                     void* stream);
/* counts[i] = #{j : |p_i - p_j|^2 < radius^2} (inclusive != 0: <=), the point itself included.
 * Open3D's RemoveRadiusOutliers keeps i when counts[i] > nb_points (strict search, inclusive = 0). */
int fnr_cloud_radius_count(const double* xyz, int64_t n, const double* lo, const double* hi, double radius,
                           int inclusive, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);
/* scikit-learn's DBSCAN(eps, min_samples).fit(X).labels_: labels[n] (-1 = noise, clusters numbered by their first core
 * point in input order, border points join the lowest-numbered adjacent cluster); n_clusters: device int32 (nullable). */
int fnr_cloud_dbscan(const double* xyz, int64_t n, const double* lo, const double* hi, double eps, int32_t min_samples,
                     int32_t* labels, int32_t* n_clusters, void* workspace, size_t workspace_bytes, void* stream);
/* Open3D's VoxelDownSample: one output point per occupied voxel (index = floor((p - (min_bound - voxel_size/2)) /
 * voxel_size)) = mean of its points (and colours; rgb / rgb_out nullable together), summed in input order.  Voxels are
 * emitted in ascending (iz, iy, ix) order (Open3D's order is unspecified).  xyz_out / rgb_out: capacity [n][3];
 * n_out: device int32 = number of occupied voxels. */
int fnr_cloud_voxel_down_sample(const double* xyz, const double* rgb, int64_t n, const double* min_bound,
                                const double* max_bound, double voxel_size, double* xyz_out, double* rgb_out,
                                int32_t* n_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- k nearest neighbours on a cloud: the Open3D calls of Nerfstudio's `pointcloud` export ----- */
/* ExportPointCloud (the `pointcloud` subcommand scripts/exporter.py:49,124-129 registers) cleans its cloud with Open3D's
 * remove_statistical_outlier(nb_neighbors=20, std_ratio) and estimate_normals(); both are kNN queries.  Clouds, lo / hi
 * and the workspace are as above (workspace >= fnr_cloud_knn_workspace_bytes(n, k)); 1 <= k <= FNR_CLOUD_KNN_MAX.
 * The search is exact and its results are functions of the input alone (csrc/cloud_knn.hip). */
#define FNR_CLOUD_KNN_MAX 32
size_t fnr_cloud_knn_workspace_bytes(int64_t n_points, int32_t k);
/* Row i of dist2 [n][k] / index [n][k] (either nullable): the k points nearest to point i, itself included, ascending
 * by squared distance ((dx*dx) + dy*dy) + dz*dz (fp64, every operation rounded), ties by ascending input index.
 * n < k: the first n entries are valid, the rest +inf / -1.  n == 0 launches nothing. */
int fnr_cloud_knn(const double* xyz, int64_t n, const double* lo, const double* hi, int32_t k, double* dist2,
                  int32_t* index, void* workspace, size_t workspace_bytes, void* stream);
/* Open3D RemoveStatisticalOutliers(nb_neighbors, std_ratio): avg_distance[n] = mean of the distances to the nb_neighbors
 * nearest points (self included); over the points with avg > 0: mean, std (n_valid - 1 in the denominator), threshold =
 * mean + std_ratio * std; keep[n] (uint8) = avg > 0 && avg < threshold; stats[3] (device) = mean, std, threshold.
 * The global sums run in a fixed order: the same cloud gives the same bits.  nb_neighbors < 1 or std_ratio <= 0: error. */
int fnr_cloud_statistical_outlier(const double* xyz, int64_t n, const double* lo, const double* hi,
                                  int32_t nb_neighbors, double std_ratio, double* avg_distance, uint8_t* keep,
                                  double* stats, void* workspace, size_t workspace_bytes, void* stream);
/* Open3D EstimateNormals(KDTreeSearchParamKNN(knn)): normals[n][3] = unit eigenvector of the smallest eigenvalue of the
 * covariance of the knn nearest points (self included); fewer than 3 of them: (0, 0, 1).  The sign is not oriented. */
int fnr_cloud_estimate_normals(const double* xyz, int64_t n, const double* lo, const double* hi, int32_t knn,
                               double* normals, void* workspace, size_t workspace_bytes, void* stream);

/* ---- second counting stage: batched template fits ---------------------------------------------- */
/* split_large_cluster (clustering/clustering_base.py:260-511) registers the fruit template to every large cluster's
 * surface with Open3D's ICP and scores six hypotheses by their Hausdorff distance.  These entry points run both for all
 * clusters of a cloud at once (csrc/cloud_fit.hip); fp64, every reduction in a fixed order, so a problem's result does
 * not depend on what else is in the batch.  Point sets are [n][3] float64 DEVICE arrays of concatenated segments; the
 * *_offsets (one more entry than segments, starting at 0, ending at the point count) and the *_id arrays are HOST
 * arrays, checked before anything is launched.  n_problems == 0 launches nothing. */
size_t fnr_cloud_icp_workspace_bytes(int64_t n_problems);
/* registration_icp(source, target, max_correspondence_distance, init, TransformationEstimationPointToPoint(
 * with_scaling), ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration)) (:262-279), Open3D's loop:
 * evaluate; then per iteration Umeyama on the current pairs, T = update * T, re-evaluate; stop when |d fitness| and
 * |d inlier_rmse| are both below the criteria, when fewer than 3 pairs remain, or at max_iteration.  The whole loop runs
 * on the device.  Problem b registers source segment src_id[b] (shared, never replicated) onto target segment b.
 * A pair needs distance < max_correspondence_distance (STRICT <); the nearest target is exact, ties go to the lowest
 * target index.  init / transformation: [n_problems][16] row-major 4 x 4; fitness, inlier_rmse: [n_problems];
 * iterations: [n_problems] = the count Open3D's loop variable ends at (the iteration that found < 3 pairs included);
 * correspondences: for problem b, one int32 per point of its source segment (target index within segment b, -1 = none),
 * problems concatenated in order.  An empty target gives fitness 0 and transformation = init. */
int fnr_cloud_icp(const double* tgt_xyz, int64_t n_tgt_points, const int64_t* tgt_offsets, int64_t n_problems,
                  const double* src_xyz, int64_t n_src_points, const int64_t* src_offsets, int64_t n_sources,
                  const int32_t* src_id, const double* init, double max_correspondence_distance, int32_t with_scaling,
                  int32_t max_iteration, double relative_fitness, double relative_rmse, double* transformation,
                  double* fitness, double* inlier_rmse, int32_t* iterations, int32_t* correspondences, void* workspace,
                  size_t workspace_bytes, void* stream);
/* n_queries: sum over the problems of |A_b| + |B_b|. */
size_t fnr_cloud_hausdorff_workspace_bytes(int64_t n_problems, int64_t n_queries);
/* hausdorff_distance(A_b, B_b, distance="euclidean") (:277, :315).  A_b = segment a_id[b] of a_xyz.  B_b is never stored:
 * it is source segment src_id[b] placed k times, point j = p * n_src + i being src[i] + translations[trans_offsets[b] +
 * p] (k = trans_offsets[b+1] - trans_offsets[b] > 0; translations: device [n_translations][3]), or, for a problem
 * without translations, src[i] under transforms[b] (device [n_problems][16] row-major 4 x 4; nullable when every problem
 * has translations; trans_offsets nullable when none has).  distances [n_problems][3] = max_a min_b |a - b|,
 * max_b min_a |a - b|, the larger of the two; witnesses [n_problems][2] = the a whose nearest b is farthest, the b
 * (index into the placed set) whose nearest a is farthest, the lowest index on ties.  The search is exact.  A problem
 * with an empty set gives NaN / -1. */
int fnr_cloud_hausdorff(const double* a_xyz, int64_t n_a_points, const int64_t* a_offsets, int64_t n_a_sets,
                        const double* src_xyz, int64_t n_src_points, const int64_t* src_offsets, int64_t n_sources,
                        int64_t n_problems, const int32_t* a_id, const int32_t* src_id, const double* translations,
                        int64_t n_translations, const int64_t* trans_offsets, const double* transforms,
                        double* distances, int32_t* witnesses, void* workspace, size_t workspace_bytes, void* stream);

/* ---- eval-image metrics ------------------------------------------------------------------------ */
/* FruitModel.get_image_metrics_and_images (fruit_nerf/fruit_nerf.py:403-458) on the device: everything the reference
 * computes with torchmetrics on a rendered [H, W, 3] image, as raw sums (the host forms the four ratios):
 *   PSNR(data_range 1, :427): squared error of clamp(rgb, 0, 1) (:408) against the image;
 *   SSIM (:428; torchmetrics defaults: 11 x 11 gaussian, sigma 1.5, k1 0.01, k2 0.03, data_range None = the larger of
 *        the value ranges of the image and of clamp(rgb, 0, 1), found on the device): the mean over the
 *        (H - 10) x (W - 10) x 3 interior values of the valid-window SSIM map (torchmetrics pads by 5 and crops the
 *        padded border away again); gauss11: HOST array of the 11 normalised float32 window weights;
 *   IoU  (:449-453): BinaryJaccardIndex(threshold 0.5) of `F.softmax(semantics)` — no dim given: on the [H, W, 1] map
 *        torch's implicit dim is 0, a softmax over image ROWS — and of sigmoid(semantics), each against mask > 0.5.
 * rgb / image: [H][W][3]; semantics (logits) / mask: [H][W], nullable together.
 * out: 8 doubles (device) = { squared error, SSIM sum, intersection | union of sigmoid > 0.5, intersection | union of the
 * row softmax > 0.5, number of SSIM values, number of squared-error terms }.
 * workspace: >= fnr_image_metrics_workspace_bytes(H, W) bytes, caller-owned.  H, W > 10. */
size_t fnr_image_metrics_workspace_bytes(int H, int W);
int fnr_image_metrics(int H, int W, const float* rgb, const float* image, const float* semantics, const float* mask,
                      const float* gauss11, double* out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRUITNERF_HIP_H */
