/*
 * nb_hip.h — C ABI of libnb_hip.so, the MI355X (gfx950) implementation of the
 * Neural Body rendering hot path.
 *
 * Conventions:
 *   - every entry point returns 0 on success, a negative NB_E* code on failure;
 *     nb_last_error() returns a thread-local description of the last failure.
 *     Nothing throws across the ABI, nothing calls exit().
 *   - all pointers marked "dev" are DEVICE pointers owned by the caller (PyTorch-ROCm
 *     tensors: tensor.data_ptr()).  The library never allocates or frees user-visible
 *     memory, links no vendor BLAS and keeps no hidden state between calls.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     work is enqueued asynchronously, no entry point synchronises the device.
 *   - floats are fp32, indices int32 unless stated.
 *
 * Each entry point names the reference interface it replaces (paths are into
 * zju3dv/neuralbody, i.e. /root/reference).
 */
#ifndef NB_HIP_H
#define NB_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NB_OK 0
#define NB_EINVAL (-1)  /* bad argument (null pointer, unsupported size) */
#define NB_ELAUNCH (-2) /* HIP launch / runtime error */
#define NB_ENODEV (-3)  /* no gfx950 device */

#define NB_ABI_VERSION 20

/* arithmetic of the decoder (nb_decode_points / nb_march `precision` argument) */
#define NB_PREC_F32 0   /* exact fp32 on v_mfma_f32_32x32x2_f32, trilinear gather of the dense volumes on the VALU: the reference's
                           own precision (the training forward, the activation tap, debugging) */
#define NB_PREC_F16F6 1 /* the default.  fc_0 FOLDED INTO THE VOLUME: trilinear interpolation and fc_0 are both linear with
                           nothing between them (latent_xyzc.py:62-72,99), so fc_0 . interp(V) = interp(fc_0 . V).
                           nb_fold_build stores U_l = fc_0[:, level l] . V_l per ACTIVE voxel (256 channels, fp16 head + fp16
                           remainder); the kernel fetches the rows of the voxels its 64 samples touch and contracts them with
                           the sparse trilinear-weight matrix Wt [voxel x sample] on the matrix pipe (three fp16 products per
                           K = 16 voxels, products exact, fp32 accumulate: fp32-level accuracy).  Needs nb_scene.fold.
                           fc_1, fc_2 and the colour head (feature_fc . latent_fc . view_fc folded into one layer): fp16 head x
                           fp16 head on v_mfma_f32_32x32x16_f16 + the two head x remainder cross terms on
                           v_mfma_scale_f32_32x32x64_f8f6f4 (weights fp4 e2m1 with a pack-time E8M0 scale per row and 32 K — fp6 e2m3
                           until ABI 19; the build flag NB_FP4_TERMS selects — activations bf6 e3m2 with a run-time E8M0 scale per
                           sample and 32 K), fp32 accumulate: ~2^-13 relative per cross term, RGB <= 4e-5 on every fixture.
                           Weight blocks whose elements span more than ~2^3 lose their small elements: see
                           nb_mlp_six_bit_stats_offset().  Rays whose LAST density it cannot sign: nb_march's ill_scratch. */

/* MLP geometry fixed by lib/networks/latent_xyzc.py:20-28 */
#define NB_FEAT_DIM 352 /* 32 + 64 + 128 + 128 interpolated channels */
#define NB_HID 256
#define NB_VIEW_HID 128
#define NB_N_LEVELS 4
#define NB_TAP_WIDTH 1600

const char *nb_last_error(void);
int nb_abi_version(void);
/* returns the number of visible HIP devices (>=0) or a negative error */
int nb_device_count(void);

/* ---------------------------------------------------------------------------------
 * Scene description shared by the decode / march entry points.
 * Mirrors `sp_input` built at lib/networks/renderer/if_clight_renderer.py:29-52 plus
 * the four feature volumes returned by Network.encode_sparse_voxels
 * (lib/networks/latent_xyzc.py:30-39).  Volumes are CHANNELS-LAST: vol[l] is a dense
 * [D_l, H_l, W_l, C_l] fp32 array (C_l = 32, 64, 128, 128), zeros at inactive voxels.
 * ------------------------------------------------------------------------------- */
/* fc_0 folded into the four latent volumes (NB_PREC_F16F6), built by nb_fold_build from the SAME volumes and fc_0 weight:
 * row r of level l = fc_0.weight[:, channels of level l] . V_l[voxel of row r]  (256 outputs) as 256 fp16 heads followed by 256
 * fp16 remainders (1 KiB); grid[l] = index grid of the level ([D_l,H_l,W_l] int32: row id inside the level or -1 = no row). */
typedef struct nb_fold {
    const uint16_t *urows;            /* dev [(rows of all levels) + 1][512]; the extra last row is all zero */
    const int32_t *grid[NB_N_LEVELS]; /* dev */
    int32_t row_base[NB_N_LEVELS];    /* first row of each level inside urows */
    int32_t zero_row;                 /* index of the all-zero row (inactive voxels, padding) */
} nb_fold;

typedef struct nb_scene {
    const float *vol[NB_N_LEVELS]; /* dev */
    int32_t vol_dhw[NB_N_LEVELS][3];
    /* dev, NB_POSE_FLOATS floats: R[9] row-major (canonical = (p_world - Th) @ R, latent_xyzc.py:41-47) | Th[3] |
     * bounds_min[3] (SMPL-space AABB minimum, xyz order = sp_input['bounds'][0]).  The per-frame tensors of sp_input
     * are read by the kernels themselves: they never visit the host, so nothing about a frame is cached host-side. */
    const float *pose;
    float voxel_size[3]; /* cfg.voxel_size, dhw order (latent_xyzc.py:54) */
    int32_t out_sh[3];   /* full-resolution grid D,H,W (sp_input['out_sh']) */
    const nb_fold *fold; /* HOST pointer or NULL; required by NB_PREC_F16F6 (which does not read vol[]) */
} nb_scene;
#define NB_POSE_FLOATS 15

/* ---------------------------------------------------------------------------------
 * Packed decoder weights.  nb_mlp_pack_size() floats; produced by nb_mlp_pack() from
 * the reference's parameter tensors (Conv1d(k=1) weights [out,in,1] viewed as [out,in]).
 * The blob holds both formats (fp32 fragments for NB_PREC_F32, the fp16 / fp4 fragment stream of NB_PREC_F16F6).
 * The packing re-orders every layer into MFMA A-operand fragment order and merges
 * feature_fc with the first 256 columns of latent_fc (no activation sits between them,
 * latent_xyzc.py:106-111).  nb_mlp_latent_bias() folds the per-frame latent code
 * (latent_xyzc.py:108-111) into that merged layer's bias; call it whenever
 * latent_index or the parameters change.
 * ------------------------------------------------------------------------------- */
int64_t nb_mlp_pack_size(void);        /* floats in the packed blob */
int64_t nb_mlp_latent_bias_size(void); /* floats in the per-frame bias block (384: see nb_mlp_latent_bias) */
/* Float offset inside the packed blob of 6 int32 counters written with the NB_PACK_F16F6 section: for each of the three
 * layers that kernel runs with narrow cross terms (fc_1, fc_2, the folded feature_fc / latent_fc / view_fc layer) {small, nonzero}
 * = how many non-zero weights lie below 1/8 of the maximum of their (row, 32 K) block — where fp6 e2m3 keeps fewer than 3 and fp4 e2m1 no
 * significant bits — and how many are non-zero at all.  small / nonzero is ~0.2 for normally distributed weights; a caller that
 * cannot rule out weight blocks with a wide dynamic range (> ~2^5) uses it to fall back to NB_PREC_F32 (the Python Network does,
 * precision "auto"). */
int64_t nb_mlp_six_bit_stats_offset(void);

typedef struct nb_mlp_params { /* all dev, row-major [out,in] / [out] */
    const float *fc0_w, *fc0_b;         /* [256,352] */
    const float *fc1_w, *fc1_b;         /* [256,256] */
    const float *fc2_w, *fc2_b;         /* [256,256] */
    const float *alpha_w, *alpha_b;     /* [1,256]   */
    const float *feature_w, *feature_b; /* [256,256] */
    const float *latent_w, *latent_b;   /* [256,384] */
    const float *view_w, *view_b;       /* [128,346] */
    const float *rgb_w, *rgb_b;         /* [3,128]   */
} nb_mlp_params;

/* replaces: module parameter access in Network.calculate_density_color
 * (lib/networks/latent_xyzc.py:99-121).  `packed` dev, nb_mlp_pack_size() floats. */
int nb_mlp_pack(const nb_mlp_params *p, float *packed, void *stream);
/* The same, writing only the sections a caller is going to use (a training step changes the weights every iteration and
 * decodes with NB_PREC_F32 only).  The fp32 section (NB_PACK_F32) is always written. */
#define NB_PACK_F32 1
#define NB_PACK_F16F6 2 /* the weight stream of NB_PREC_F16F6 (fc_1, fc_2, the folded colour head; fc_0 lives in nb_fold) */
#define NB_PACK_ALL 3
int nb_mlp_pack_sections(const nb_mlp_params *p, float *packed, int sections, void *stream);
/* latent_row: dev pointer to latent.weight[latent_index] (128 floats);
 * out: dev, nb_mlp_latent_bias_size() floats = [256: bias of the merged feature_fc / latent_fc layer with the latent code
 * folded in | 128: bias of view_fc with that layer folded in as well (feature_fc, latent_fc and view_fc have no activation
 * between them, latent_xyzc.py:105-119; NB_PREC_F16F6 runs them as one layer)], MFMA fragment order. */
int nb_mlp_latent_bias(const nb_mlp_params *p, const float *latent_row, float *out, void *stream);

/* ---------------------------------------------------------------------------------
 * nb_fold_build — the encoder-side half of NB_PREC_F16F6: replaces the first decoder layer's weight access in
 * Network.calculate_density_color (lib/networks/latent_xyzc.py:99, `self.fc_0(features)`) together with the four
 * F.grid_sample calls feeding it (:62-72), by pre-multiplying every ACTIVE voxel of the four volumes with fc_0.
 *   vol[l] dev channels-last [D_l,H_l,W_l,C_l] fp32 (nb_scene.vol); rows_lin[l] dev [n_rows_max[l]] int32: linear voxel index
 *   of each active row — or rows_lin[l] NULL: vol[l] then holds the level's ACTIVE ROWS themselves, compact [n_rows_max[l], C_l]
 *   (what the encoder produces before `.dense()`, latent_xyzc.py:188-201: no dense volume need exist for this arithmetic);
 *   n_rows[l] dev [1] int32 (device-side count, <= n_rows_max[l]); fc0_w dev [256,352] fp32 row-major;
 *   urows dev [(sum of n_rows_max) + 1][512] uint16: level l's rows start at row sum_{k<l} n_rows_max[k]; the last row is
 *   zero-filled by the call (sum of n_rows_max < 2^21).  Exact fp32 products (v_mfma_f32_32x32x2_f32), then head = fp16(u),
 *   remainder = fp16(u - head).  n_saturated dev [1] int32 or NULL, ZEROED BY THE CALLER (the call adds to it; the
 *   encoder's one zero fill covers it): zero iff no product of a live row was beyond the fp16 range (+-65504: clamped) or not
 *   finite (a NaN product stays NaN in the planes), otherwise a positive lower bound of their number (the lanes that saw one, not
 *   the products) — the planes then do not carry fc_0 . V, use NB_PREC_F32 for such weights / volumes.
 * nb_sparsify — active set of a DENSE volume that did not come with one (volumes handed to Network.calculate_density_color by a
 * caller other than encode_sparse_voxels): a voxel is active iff any channel is non-zero.  grid dev [D*H*W] int32 out (row id
 * or -1), rows_lin dev [n_rows_max] out (linear-voxel order), n_rows dev [1] out (clamped to n_rows_max; rows beyond it are
 * dropped: size n_rows_max = D*H*W to be safe); scratch dev nb_scan_scratch_size(D*H*W) bytes.
 * ------------------------------------------------------------------------------- */
int nb_fold_build(const float *const vol[NB_N_LEVELS], const int32_t *const rows_lin[NB_N_LEVELS],
                  const int32_t *const n_rows[NB_N_LEVELS], const int32_t n_rows_max[NB_N_LEVELS], const float *fc0_w,
                  uint16_t *urows, int32_t *n_saturated, void *stream);
int nb_sparsify(const float *vol, const int32_t dhw[3], int32_t c, int32_t *grid, int32_t *rows_lin, int32_t *n_rows,
                int32_t n_rows_max, void *scratch, void *stream);

/* ---------------------------------------------------------------------------------
 * nb_decode_points — replaces Network.calculate_density_color
 * (lib/networks/latent_xyzc.py:91-126) and, with density_only != 0,
 * Network.calculate_density (:74-89).
 *   wpts    dev [n,3] world-space points; viewdir dev [n,3] (ignored when density_only)
 *   raw_out dev [n,4] (rgb logits, sigma)   or [n,1] sigma when density_only
 *   dbg     dev or NULL (NB_PREC_F32 only): activation tap, NB_TAP_WIDTH floats per point:
 *           [F 352 | h1 256 | h2 256 | h3 256 | G 256 (latent_fc output) | V 128 | PE 90 | pad]
 *           (post-ReLU where the layer has one) — what the backward pass consumes; also used by tests
 * ------------------------------------------------------------------------------- */
int nb_decode_points(const nb_scene *scene, const float *packed, const float *latent_bias,
                     const float *wpts, const float *viewdir, int64_t n, int density_only,
                     float *raw_out, float *dbg, int precision, void *stream);

/* ---------------------------------------------------------------------------------
 * Optional sample culling of nb_march — replaces prepare_inside_pts of the mask-culled renderers
 * (lib/networks/renderer/if_clight_renderer_mmsk.py:12-45, if_clight_renderer_msk.py:12-49): a sample
 * is decoded only if it projects inside every one of n_views silhouettes; culled samples get raw = 0
 * (if_clight_renderer_mmsk.py:54-59).  pre_affine != 0 (the _msk variant) first maps the point
 * world -> SMPL space of the rendered pose (scene R, Th) -> world of the snapshot frame (R0, Th0).
 * Arithmetic, fp32: every row of a 3x3 product is the ascending FMA chain fma(p2, m2, fma(p1, m1, p0 * m0)) — what the
 * reference's matrix products evaluate to on the CPU —, a translation is a separate add, the perspective division IEEE;
 * the pixel is rint (half to even) clamped to the mask, a coordinate that is not finite or beyond 9e18 reads pixel 0.
 * ------------------------------------------------------------------------------- */
#define NB_SLOT_DEAD (-2147483647 - 1) /* nb_march ray_order: empty slot */
#define NB_MAX_CULL_VIEWS 64 /* the reference loops over batch['Ks'].size(1) training views (4 or 6 in the shipped configs) */
#define NB_CULL_CAM_FLOATS 21
typedef struct nb_cull {
    int32_t n_views;    /* 1..NB_MAX_CULL_VIEWS */
    int32_t H, W;       /* mask size = int(cfg.H * cfg.ratio), int(cfg.W * cfg.ratio) */
    int32_t pre_affine;
    const uint8_t *msk; /* dev [n_views,H,W] uint8, non-zero = inside (batch['msks'][0] / batch['msk']) */
    const float *cam;   /* dev [n_views, NB_CULL_CAM_FLOATS]: row-major 3x4 [R|T] (batch['RT']) | K 3x3 (batch['Ks'] / batch['K']) */
    const float *snap;  /* dev 12 floats: batch['R0_snap'] (9) | batch['Th0_snap'] (3); NULL unless pre_affine */
} nb_cull;

/* ---------------------------------------------------------------------------------
 * nb_march — the fused per-ray path (both precisions serve sample culling and the raw output): replaces Renderer.get_pixel_value
 * (lib/networks/renderer/if_clight_renderer.py:62-92), i.e. get_sampling_points (:11-27),
 * get_density_color (:54-60), Network.calculate_density_color and raw2outputs
 * (lib/networks/renderer/nerf_net_utils.py:6-51, raw_noise_std = 0), for ALL rays of a
 * batch element in one launch (the reference's 2048-ray chunk loop :107-118 disappears).
 *   ray_o, ray_d dev [n_rays,3]; near, far dev [n_rays]
 *   t_vals  dev [n_samples]  = torch.linspace(0,1,n_samples)   (if_clight_renderer.py:13)
 *   t_rand  dev [n_rays,n_samples] in [0,1) or NULL            (stratified jitter, :16-23)
 *   ray_order dev [n_slots] int32 or NULL (n_slots ignored, slot i = ray i): WHICH rays march together.  64 consecutive slots
 *           share a workgroup (whose voxel list is the union of what its samples touch: the caller groups neighbouring
 *           pixels, e.g. 8 x 8 tiles).  Entry v >= 0: the slot marches ray v and stores its results at the ray's own index;
 *           v = -(r + 1) in (NB_SLOT_DEAD, 0): a padding slot that marches ray r's data and stores nothing (keeps a partially
 *           filled tile's group together); NB_SLOT_DEAD: an empty slot — a group of 64 (aligned) slots is either free of
 *           them or consists of them (it is skipped).  Every ray must appear exactly once as v >= 0.  n_slots % 64 == 0.
 *   cull    HOST pointer to an nb_cull (whose msk / cam / snap members are DEVICE pointers) or NULL (no culling)
 *   outputs dev: rgb_map [n_rays,3], disp_map/acc_map/depth_map [n_rays],
 *           weights [n_rays,n_samples]; raw (optional, may be NULL) [n_rays,n_samples,4]
 *   ill_scratch dev, ill_scratch_bytes = NB_ILL_SCRATCH_BYTES(cap) for a list of `cap` >= 1 rays (16-byte aligned), or NULL / 0;
 *           NB_PREC_F16F6 only (NB_PREC_F32 ignores it).  The reference
 *           gives a ray's LAST sample the interval 1e10 (nerf_net_utils.py:28), so that sample's alpha is a step function of the SIGN
 *           of its density; NB_PREC_F16F6's density error (~3e-4 absolute on the bench scene) can put a ray whose last density is
 *           that close to zero on the other side of the step (~4e-6 of the rays, each off by up to its remaining transmittance).  With
 *           the scratch the march LISTS every ray whose last density is within NB_ILL_SIGMA of zero while its transmittance in front
 *           of that sample exceeds NB_ILL_T_MIN (state in front of the sample + the sample's colour logits, <= cap rays), and a
 *           second small kernel on the same stream recomputes that one density per listed ray at fp32 level (fc_0 through the folded
 *           planes' head + remainder pairs, fc_1 / fc_2 / alpha_fc from the fp32 section of `packed`, fp64 accumulation), composites
 *           the last sample again and rewrites the ray's rgb / disp / acc / depth, weights[n_samples - 1] and raw[n_samples - 1][3].
 *           No host read-back.  Afterwards the scratch starts with int32 {rays listed (may exceed cap: the excess keeps the
 *           march's result), rays whose step changed side}.  The call zeroes that header itself.  NULL: the march's result as is.
 *           The bench view lists ~50 of its 262 144 rays (~20 us); a cap of a few thousand covers any trained scene, whose empty
 *           space has a strongly negative density — only a decoder whose density is ~0 over whole regions lists rays by the
 *           thousand (12 533 listed rays: +0.5 ms), which is what the cap bounds.
 * ------------------------------------------------------------------------------- */
#define NB_ILL_SIGMA 4e-3f  /* > 10 x the measured density error of NB_PREC_F16F6 on the bench scene (alpha_fc weights x 50) */
#define NB_ILL_T_MIN 1e-6f  /* a last sample in front of which less transmittance is left cannot move the ray by more */
#define NB_ILL_HEADER_FLOATS 16
#define NB_ILL_RECORD_FLOATS 16
#define NB_ILL_FIXUP_BLOCKS 1024
#define NB_ILL_SCRATCH_BYTES(cap) (4 * ((int64_t)NB_ILL_HEADER_FLOATS + (int64_t)(cap) * NB_ILL_RECORD_FLOATS))
int nb_march(const nb_scene *scene, const float *packed, const float *latent_bias,
             const float *ray_o, const float *ray_d, const float *near, const float *far,
             int64_t n_rays, int32_t n_samples, const float *t_vals, const float *t_rand,
             const int32_t *ray_order, int64_t n_slots, const nb_cull *cull, int white_bkgd, float *rgb_map, float *disp_map, float *acc_map, float *weights,
             float *depth_map, float *raw, void *ill_scratch, int64_t ill_scratch_bytes, int precision, void *stream);

/* ---------------------------------------------------------------------------------
 * nb_composite — raw2outputs alone (lib/networks/renderer/nerf_net_utils.py:6-51) for
 * callers that decode points themselves (the _mmsk/_msk renderers).
 *   raw dev [n_rays,n_samples,4]; z_vals dev [n_rays,n_samples]; ray_d dev [n_rays,3]
 * ------------------------------------------------------------------------------- */
int nb_composite(const float *raw, const float *z_vals, const float *ray_d, int64_t n_rays,
                 int32_t n_samples, int white_bkgd, float *rgb_map, float *disp_map,
                 float *acc_map, float *weights, float *depth_map, void *stream);

/* ---------------------------------------------------------------------------------
 * Backward pass (training step: lib/train/trainers/if_nerf_clight.py:18-36 runs Renderer.render
 * under autograd; the reference's backward is PyTorch autograd through the same modules).
 * ------------------------------------------------------------------------------- */

/* d raw [n_rays,n_samples,4] from d rgb_map [n_rays,3] (and optionally d acc_map / d depth_map
 * [n_rays], may be NULL): backward of raw2outputs (nerf_net_utils.py:19-49, raw_noise_std 0). */
int nb_composite_bwd(const float *raw, const float *z_vals, const float *ray_d, int64_t n_rays,
                     int32_t n_samples, int white_bkgd, const float *d_rgb_map, const float *d_acc_map,
                     const float *d_depth_map, float *d_raw, void *stream);

/* nb_composite_bwd_maps — the backward of raw2outputs (nerf_net_utils.py:19-49) for ALL five of its outputs: replaces what autograd
 * does in the reference when a loss reads acc_map (the wrapper's acc_crit, lib/train/trainers/if_nerf_clight.py:16), depth_map,
 * disp_map or weights.  The arguments of nb_composite_bwd plus d_disp_map dev [n_rays] and d_weights dev [n_rays, n_samples].  Any
 * of the five cotangents may be NULL, read as 0; at least one must be given (NB_EINVAL otherwise); n_rays == 0: NB_OK at once.
 * One thread per ray, two sweeps (T_i stashed in d_raw[..., 3] by the first), with c = sigmoid(raw_rgb), B_i = sum_{k>i} w_k dw_k:
 *   dw_i     = g_rgb . c_i + g_acc + g_depth z_i - [white_bkgd] sum(g_rgb) + d_weights[ray, i]
 *   d raw_rgb = w_i g_rgb (.) c_i (1 - c_i)
 *   dalpha_i = T_i dw_i - B_i / (1 - alpha_i + 1e-10)
 *   dsigma_i = dalpha_i dist_i (1 - alpha_i) [sigma_i > 0]
 * With only d_rgb_map / d_acc_map / d_depth_map given, d_raw is nb_composite_bwd's bit for bit (the same operations in the same order).
 * Disparity: disp = 1 / max(1e-10, q) with q = depth / acc (nerf_net_utils.py:42-43).  The first sweep also forms acc = sum w_i and
 * depth = sum w_i z_i (fp32, in sample order).  Where q > 1e-10 the two scalars become
 *   g_acc += d_disp / (q acc)      g_depth -= d_disp / (q q acc)
 * Where q is NOT greater than 1e-10 — a smaller value, a tie, or NaN (acc == 0: every density <= 0, the usual background ray) —
 * d_disp_map contributes nothing.  Autograd gives NaN there (0 * NaN through depth / acc); this entry gives 0. */
int nb_composite_bwd_maps(const float *raw, const float *z_vals, const float *ray_d, int64_t n_rays, int32_t n_samples,
                          int white_bkgd, const float *d_rgb_map, const float *d_acc_map, const float *d_depth_map,
                          const float *d_disp_map, const float *d_weights, float *d_raw, void *stream);

/* nb_ray_distortion — compactness of a ray's weights; no counterpart in the reference (its floaters are removed from the mesh after
 * the fact).  It is the distortion loss of Mip-NeRF 360 restated for this renderer's samples: sample i stands for the interval up to
 * the next sample, as raw2outputs uses it; the last sample is a point at the far end.
 *   weights, z_vals dev [n_rays, n_samples] (z non-decreasing along a ray) -> loss dev [n_rays], d_weights dev [n_rays, n_samples]
 *   or NULL (not computed).  Per ray, with span = z[S-1] - z[0]:
 *   span not greater than 0 (one sample, near == far, NaN): loss = 0 and d_weights = 0.  Otherwise s_i = (z_i - z_0) / span,
 *   m_i = (s_i + s_{i+1}) / 2 and delta_i = s_{i+1} - s_i for i < S-1, m_{S-1} = s_{S-1} and delta_{S-1} = 0,
 *     L   = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i
 *     G_k = dL / dw_k = 2 sum_j w_j |m_k - m_j| + (2/3) w_k delta_k
 *   in O(S) per ray from running sums of w_j and w_j m_j (m is non-decreasing; csrc/nb_ray_loss.hip has the order).  The fp32 inputs
 *   are converted exactly to float64; s, m, delta and every sum are float64; loss and G are rounded to fp32 once, on store.  No
 *   atomics: the same inputs give the same bits.  z_vals gets no gradient (sample depths are constants of the training step).
 *   1 <= n_samples <= 512 (the importance pass's S + N ceiling), n_rays >= 0, else NB_EINVAL; n_rays == 0: NB_OK at once. */
int nb_ray_distortion(const float *weights, const float *z_vals, int64_t n_rays, int32_t n_samples, float *loss, float *d_weights,
                      void *stream);

/* Row-major fp32 GEMM C[m,n] = alpha * op(A) op(B) + beta * C on the fp32 matrix cores (v_mfma_f32_32x32x2_f32, exact
 * fp32): the backward of the Conv1d(k=1) layers (latent_xyzc.py:99-121).  lda/ldb/ldc are row strides.  op(A) = A^T
 * (trans_a) is the weight-gradient form dW = dY^T X (split over the long row dimension, fp32 atomics; for M, N >= 32, K >= 1024
 * and 16-byte aligned rows it runs on the 16-bit matrix pipe with both operands as bf16 head + remainder pairs, ~2^-16
 * relative, else exact fp32; op(B) = B only:
 * trans_a && trans_b is refused with NB_EINVAL, no caller of the path needs it).  Summation order: the trans_a form and the
 * colsum epilogue of nb_gemm_fused accumulate with fp32 atomics, so weight / bias gradients are reproducible to rounding
 * (~1e-7 relative), not bit for bit, from run to run — like the reference's own cuBLAS / atomics-based backward.  k == 0 is
 * an empty product: C = beta C (and the epilogue); m == 0 or n == 0 is an empty result: NB_OK at once, no pointer is looked at. */
int nb_sgemm(int trans_a, int trans_b, int32_t m, int32_t n, int32_t k, float alpha, const float *a, int32_t lda,
             const float *b, int32_t ldb, float beta, float *c, int32_t ldc, void *stream);
/* (The non-transposed-A form with op(B) = B, >= 1024 rows, K a multiple of 32 and 16-byte aligned operands — the dX = dY . W
 * products — also runs on the 16-bit matrix pipe with bf16 pairs.)
 * The same with the epilogues of the backward chain fused (trans_a = 0 only):
 *   mask_y (dev [m, >= n], row stride ldy, or NULL): C[r,c] = 0 where mask_y[r,c] <= 0 — the ReLU that followed the
 *            layer whose input gradient C is (mask_y = that layer's post-activation output);
 *   colsum (dev [n] or NULL): colsum[c] += sum_r C[r,c] after the mask — the bias gradient of that layer. */
int nb_gemm_fused(int trans_a, int trans_b, int32_t m, int32_t n, int32_t k, float alpha, const float *a, int32_t lda,
                  const float *b, int32_t ldb, float beta, float *c, int32_t ldc, const float *mask_y, int32_t ldy,
                  float *colsum, void *stream);

/* Which kernel nb_gemm_fused / nb_sgemm launches for these arguments (host only, launches nothing; a and b count for their
 * alignment only and are never dereferenced; NB_BWD_SPLIT is honoured as the launch honours it): 0 = none, op(A) = A^T with k == 0
 * (C = beta C), 1 = split-K fp32 (op(A) = A^T), 2 = split-K bf16 pairs, 3 = the general fp32 kernel, 4 = the aligned fp32 kernel,
 * 5 = the aligned fp32 kernel with op(B) = B^T, 6 = bf16 pairs (>= 1024 rows).  Sizes and flags are not validated here. */
int nb_gemm_variant(int trans_a, int trans_b, int32_t m, int32_t n, int32_t k, const float *a, int32_t lda, const float *b,
                    int32_t ldb);

/* dy[i] = y[i] > 0 ? dy[i] : 0 (ReLU backward on the post-activation value), in place. */
int nb_relu_bwd(float *dy, const float *y, int64_t n, void *stream);
/* out[c] += sum_r x[r*ld + c]  (bias gradients); out must be initialised by the caller. */
int nb_colsum(const float *x, int64_t n_rows, int32_t n_cols, int32_t ld, float *out, void *stream);

/* Backward of the 4-level trilinear lookup (F.grid_sample, latent_xyzc.py:62-72) restricted to the
 * ACTIVE voxels: d_feat dev [n,352] -> drows[l] dev [n_rows_l, C_l] (+=, atomics; zero them first),
 * grids[l] dev = index grid of level l (row id or -1).  scene->vol[] is not read.
 * run_length >= 1: consecutive points [k run_length, (k+1) run_length) are the samples of ONE ray in depth order (the training
 * step: N_samples); contributions to the same base voxel are summed along such a run before they are added atomically (the
 * result is the same sum in another order).  1 = every point on its own. */
int nb_trilinear_bwd(const nb_scene *scene, const int32_t *const grids[4], float *const drows[4],
                     const float *wpts, const float *d_feat, int64_t n, int32_t run_length, void *stream);

/* ---------------------------------------------------------------------------------
 * Structured-latent-code encoder — replaces Network.encode_sparse_voxels
 * (lib/networks/latent_xyzc.py:30-39) + SparseConvNet.forward (:184-205) and the spconv
 * v1.2.1 calls inside (SubMConv3d / SparseConv3d / BatchNorm1d / ReLU / .dense()).
 * A sparse tensor is (rows [n,C] fp32, coords [n] linear voxel index, index grid
 * [D,H,W] int32 holding the row id or -1).
 * ------------------------------------------------------------------------------- */

/* Voxelise the SMPL vertices: dedup (last vertex index wins, spconv_standin rule),
 * build the index grid and compact row list.
 *   coord dev [n_verts,3] (d,h,w) int32; grid dev [D*H*W] int32 (overwritten; filled with -1 by the call unless flags has
 *   NB_GRID_PREFILLED);
 *   rows_vert dev [n_verts] int32 out: vertex id feeding each row; rows_lin dev [n_verts]
 *   int32 out: linear voxel index of each row; n_rows dev [1] int32 out.
 *   scratch dev: at least nb_scan_scratch_size(n_verts) bytes. */
int64_t nb_scan_scratch_size(int64_t n);
#define NB_GRID_PREFILLED 1 /* flags of nb_enc_voxelize / nb_enc_downsample_index: the caller filled the index grid with -1 (one fill
                               for the grids of all five levels of an encoder pass instead of one memset each) */
int nb_enc_voxelize(const int32_t *coord, int32_t n_verts, const int32_t dhw[3], int32_t *grid,
                    int32_t *rows_vert, int32_t *rows_lin, int32_t *n_rows, void *scratch, int32_t flags,
                    void *stream);

/* Output active set of SparseConv3d(k=3, s=2, p=1) (latent_xyzc.py:265-274): every output
 * site with >=1 active input in its 3^3 receptive field, rows numbered in linear-voxel
 * order.  in_lin dev [n_in_max] with *n_in valid (device count); out grid dev [Do*Ho*Wo]. */
int nb_enc_downsample_index(const int32_t *in_lin, const int32_t *n_in, int32_t n_in_max,
                            const int32_t in_dhw[3], const int32_t out_dhw[3], int32_t *out_grid,
                            int32_t *out_lin, int32_t *n_out, int32_t n_out_max, void *scratch, int32_t flags,
                            void *stream);
/* The index sets of n_levels (<= NB_DOWN_LEVELS_MAX) SUCCESSIVE strided levels below a voxelised level in three launches instead of
 * three per level: level l's out_dhw is the l-fold floor((d - 1) / 2) + 1 of in_dhw; out_grid[l], out_lin[l], n_out[l], n_out_max[l] (host
 * arrays of device pointers / capacities) as in nb_enc_downsample_index.  A cell c of level l is active iff an active voxel p of the
 * base level lies within [2^l c - (2^l - 1), 2^l c + (2^l - 1)] in every coordinate: the per-level rule composed, and the same
 * cells, rows and order as n_levels chained nb_enc_downsample_index calls as long as no capacity clamps (the capacities of
 * ops.down_capacity are upper bounds).  scratch: nb_scan_scratch_size(max(cells of level 1, 64)) bytes. */
#define NB_DOWN_LEVELS_MAX 4
int nb_enc_downsample_index_all(const int32_t *in_lin, const int32_t *n_in, int32_t n_in_max, const int32_t in_dhw[3],
                                int32_t n_levels, int32_t *const out_grid[], int32_t *const out_lin[], int32_t *const n_out[],
                                const int32_t n_out_max[], void *scratch, int32_t flags, void *stream);

/* One sparse 3x3x3 convolution (stride 1 submanifold or stride 2) without bias:
 *   out[r, :] = sum_o W[o] . in[nbr(r, o), :]   over ACTIVE neighbours
 * and per-channel sum / sum of squares of the result rows (fp64) for BatchNorm.
 *   weight dev [3,3,3,Cin,Cout] (spconv 1.x layout); in_rows dev [n_in,Cin];
 *   in_grid dev index grid of the INPUT tensor; out_lin dev [n_out_max] linear voxel index
 *   of each OUTPUT row in the OUTPUT grid; n_out dev [1]; stats dev [2*Cout] fp64 (zeroed
 *   by the call unless flags has NB_CONV_STATS_ZEROED: the caller cleared it, e.g. one memset for the statistics of all
 *   17 layers instead of one launch per layer). */
#define NB_CONV_STATS_ZEROED 1
#define NB_CONV_BF16 2 /* nb_enc_conv16 only: the split operands are bf16 pairs (nb_enc_conv_pack16 mode 1, nb_enc_bn_relu_bwd dx_split) */
int nb_enc_conv(const float *in_rows, const int32_t *in_grid, const int32_t in_dhw[3],
                const int32_t *out_lin, const int32_t *n_out, int32_t n_out_max,
                const int32_t out_dhw[3], int32_t stride, const float *weight, int32_t cin,
                int32_t cout, float *out_rows, double *stats, int32_t flags, void *stream);

/* BatchNorm1d(eps=1e-3) over active rows + ReLU, in place (latent_xyzc.py:208-274).
 * training != 0: normalise with the batch statistics in `stats` (biased variance), write
 * [mean | biased var | n_rows] (2*C+1 floats) to batch_stats (dev, may be NULL when momentum < 0)
 * and, when momentum >= 0, update running_mean / running_var in place like nn.BatchNorm1d
 * (unbiased variance, latent_xyzc.py:215 momentum 0.01);
 * training == 0: use running_mean / running_var.
 * dense (dev or NULL): channels-last [D,H,W,C] volume receiving the rows (.dense(),
 * latent_xyzc.py:189-201); it must have been zero-filled by the caller.
 * rows_out (dev or NULL): when given, the activated rows go there and `rows` keeps the raw
 * convolution output (needed by nb_enc_bn_relu_bwd). */
int nb_enc_bn_relu(float *rows, const int32_t *n_rows, int32_t n_rows_max, int32_t c,
                   const double *stats, const float *gamma, const float *beta,
                   float *running_mean, float *running_var, int training, float eps, float momentum,
                   float *batch_stats, const int32_t *rows_lin, float *dense, float *rows_out, void *stream);

/* ---- the same convolution on the 16-bit matrix pipe (inference: no backward record) ----
 * Operands as fp16 head + fp16 remainder, three products per K chunk on v_mfma_f32_32x32x16_f16 with fp32 accumulation
 * (~2^-21 relative per product), 1.3-1.9x faster than nb_enc_conv.  cin in {32, 64, 128}, cout in {32, 64, 128}.
 *   nb_enc_conv_pack16: weight dev [3,3,3,Cin,Cout] fp32 -> packed dev, 27*Cin*Cout*2 uint16 (MFMA B-fragment order).
 *     mode 0: the forward convolution, fp16 pairs.  mode 1: the BACKWARD-INPUT convolution of a layer as a
 *     convolution of its own (d in[q] = sum_o d out[q + o - 1] . W[26 - o]^T: mirrored offsets, transposed slabs), bf16 pairs
 *     (gradients span more binades than an un-scaled fp16 head holds): `cin`, `cout` are those of the packed convolution =
 *     the layer's Cout, Cin; `weight` is the layer's weight [3,3,3,cout,cin].  Run it with nb_enc_conv16(flags = NB_CONV_BF16)
 *     on the bf16 planes nb_enc_bn_relu_bwd writes (dx_split), in_grid = the layer's output grid, out_lin = its input rows.
 *   nb_enc_bn_relu_split: nb_enc_bn_relu whose activated rows leave as TWO fp16 planes in rows_split (dev, 2*n_rows_max*c
 *     uint16 = the bytes of an fp32 [n_rows_max, c] matrix: heads, then remainders); `rows` (the raw convolution output) is
 *     only read; dense as in nb_enc_bn_relu; rows_out (dev or NULL): the activated rows in fp32 as well (the training
 *     forward keeps them for nb_enc_bn_relu_bwd / nb_enc_conv_bwd_weight while the next convolution reads the planes)
 *   nb_enc_conv16: in_split = such a pair of planes with in_rows_cap rows each; everything else as nb_enc_conv, and
 *     stride = -2: the TRANSPOSED gather of a stride-2 layer (its backward-input product with a mode-1 pack): output row p (a row
 *     of the layer's input level) takes, under offset k, the row of voxel (p - 1 + k) / 2 of in_grid (the layer's output grid)
 *     where that division is exact in all three coordinates.  Channel pairs: (32,32) (32,64) (64,32) (64,64) (64,128) (128,64)
 *     (128,128) */
int nb_enc_conv_pack16(const float *weight, int32_t cin, int32_t cout, uint16_t *packed, int32_t mode, void *stream);
/* up to NB_PACK_BATCH_MAX nb_enc_conv_pack16 jobs in ONE launch (host arrays of device pointers and sizes): a training step re-packs
 * every >= 32-channel convolution after each optimiser step, forward (mode 0) and backward-input (mode 1) forms */
#define NB_PACK_BATCH_MAX 32
int nb_enc_conv_pack16_batch(int32_t n_jobs, const float *const weight[], const int32_t cin[], const int32_t cout[],
                             uint16_t *const packed[], const int32_t mode[], void *stream);
int nb_enc_bn_relu_split(const float *rows, const int32_t *n_rows, int32_t n_rows_max, int32_t c,
                         const double *stats, const float *gamma, const float *beta,
                         float *running_mean, float *running_var, int training, float eps, float momentum,
                         float *batch_stats, const int32_t *rows_lin, float *dense, uint16_t *rows_split, float *rows_out,
                         void *stream);
int nb_enc_conv16(const uint16_t *in_split, int32_t in_rows_cap, const int32_t *in_grid, const int32_t in_dhw[3],
                  const int32_t *out_lin, const int32_t *n_out, int32_t n_out_max, const int32_t out_dhw[3],
                  int32_t stride, const uint16_t *wpacked, int32_t cin, int32_t cout, float *out_rows, double *stats,
                  int32_t flags, void *stream);
/* Which forward kernel nb_enc_conv16 runs for a channel pair and a row CAPACITY (host only, launches nothing): 0 = offsets split over
 * 8 waves, 1 = weight slab through LDS with every channel tile per wave, 2 = ... with two channel tiles per wave, 3 = per-wave
 * operands with every channel tile per wave, 4 = ... with one channel tile per wave; -1: not a pair of nb_enc_conv16. */
int nb_enc_conv16_variant(int32_t cin, int32_t cout, int32_t n_out_max);

/* ---- encoder backward (training).  Shapes as in the forward calls above. ---- */

/* BatchNorm1d (batch statistics) + ReLU backward.  dy, y (activated rows), x (raw conv output) dev
 * [n_rows, c]; batch_stats dev [2c+1] as written by nb_enc_bn_relu; sums dev [2c] fp64 scratch.
 * Outputs: dx dev [n_rows, c] (may alias dy), dgamma / dbeta dev [c]; dx_split (dev or NULL): dx once more as two bf16
 * planes [2, n_rows_max, c] (heads | remainders) for the backward-input convolution on the matrix pipe. */
#define NB_BWD_RULEBOOK_READY 2 /* nb_enc_conv_bwd_weight: `rulebook` already holds nbr(r, o) of this (in_grid, out_lin, stride) — written by
                                  an earlier call for a layer of the same level (its submanifold layers share one table) */
#define NB_BWD_ZEROED 1 /* flags of nb_enc_bn_relu_bwd / nb_enc_conv_bwd_weight: the caller cleared `sums` / `dweight` (one zero fill
                           for the accumulators of a whole backward pass instead of one memset per layer) */
int nb_enc_bn_relu_bwd(const float *dy, const float *y, const float *x, const int32_t *n_rows,
                       int32_t n_rows_max, int32_t c, const float *batch_stats, float eps, const float *gamma,
                       double *sums, float *dx, float *dgamma, float *dbeta, uint16_t *dx_split, int32_t flags, void *stream);

/* Gradient of the conv INPUT rows: din[q] = sum_o dx[r(q,o)] @ W[o]^T, where r(q,o) is the output row that
 * read input voxel q under kernel offset o.  out_grid = index grid of the OUTPUT tensor, in_lin = linear voxel
 * index of each INPUT row. */
int nb_enc_conv_bwd_input(const float *dx, const int32_t *out_grid, const int32_t out_dhw[3], const int32_t *in_lin,
                          const int32_t *n_in, int32_t n_in_max, const int32_t in_dhw[3], int32_t stride,
                          const float *weight, int32_t cin, int32_t cout, float *din, void *stream);

/* Gradient of the conv weight [3,3,3,Cin,Cout] (zeroed by the call unless flags has NB_BWD_ZEROED): dW[o] = sum_r in[nbr(r,o)]^T (x) dx[r].
 * rulebook: dev int32 scratch [n_out_max * 27] (receives nbr(r,o), -1 = no active input voxel; only read with NB_BWD_RULEBOOK_READY).
 * dx_split (dev or NULL): dx as bf16 head / remainder planes [2, n_out_max, Cout] (nb_enc_bn_relu_bwd writes them); when given
 * and Cin >= 32 the product runs on the 16-bit matrix pipe with both operands as bf16 pairs (three products, fp32 accumulate,
 * ~2^-16 relative) instead of the exact-fp32 MFMA kernel. */
int nb_enc_conv_bwd_weight(const float *in_rows, const int32_t *in_grid, const int32_t in_dhw[3],
                           const int32_t *out_lin, const int32_t *n_out, int32_t n_out_max, const int32_t out_dhw[3],
                           int32_t stride, const float *dx, const uint16_t *dx_split, int32_t cin, int32_t cout,
                           float *dweight, int32_t *rulebook, int32_t flags, void *stream);

/* Embedding-lookup backward: dcodes[rows_vert[r], :] = drows[r, :] (dcodes zeroed by the caller). */
int nb_enc_scatter_codes_bwd(const float *drows, const int32_t *rows_vert, const int32_t *n_rows, int32_t n_rows_max,
                             int32_t c, float *dcodes, void *stream);

/* Embedding lookup of the per-vertex codes (latent_xyzc.py:33-34): rows[r,:] = c[rows_vert[r],:] */
int nb_enc_gather_codes(const float *codes, const int32_t *rows_vert, const int32_t *n_rows,
                        int32_t n_rows_max, int32_t c, float *rows, void *stream);

/* ---------------------------------------------------------------------------------
 * nb_raygen — replaces lib/utils/render_utils.py:120-137 (image_rays), i.e. get_rays
 * (lib/utils/if_nerf/if_nerf_data_utils.py:8-21) + get_near_far (:54-69) + compaction by
 * mask_at_box, on device.  K, R (row-major 3x3) and T (3) are HOST doubles.
 *   bounds: host float[6] world-space AABB (min xyz, max xyz)
 *   outputs dev: ray_o, ray_d [H*W,3]; near, far [H*W] (first *n_rays rows valid, pixel
 *   order preserved); mask_at_box [H*W] uint8; n_rays dev [1] int32.
 *   scratch dev: nb_scan_scratch_size(H*W) bytes. */
int nb_raygen(int32_t H, int32_t W, const double K[9], const double R[9], const double T[3],
              const float bounds[6], float *ray_o, float *ray_d, float *near, float *far,
              uint8_t *mask_at_box, int32_t *n_rays, void *scratch, void *stream);

/* ---------------------------------------------------------------------------------
 * nb_train_rays — replaces the train branch of sample_ray_h36m / sample_ray
 * (lib/utils/if_nerf/if_nerf_data_utils.py:153-219 / :72-137, called per item by lib/datasets/light_stage/
 * multi_view_dataset.py:154 and monocular_dataset.py) on device: one batch of n_rays training rays drawn from a resident
 * image and mask, with get_rays (:8-21), the 2-D bound mask (:40-51) and get_near_far (:54-69) folded in.
 *   K, R (row-major 3x3), T (3): HOST doubles; bounds: host float[6] world AABB (can_bounds: min xyz, max xyz).
 *   hull_xy HOST int32 [n_hull,2] (x, y), n_hull in 3..8: the convex hull of the box's eight projected, rounded corners,
 *     counter-clockwise (train_rays.bound_hull); a pixel centre inside or on it is in the bound mask (edge functions in int64).
 *   msk dev [H*W] uint8, img dev [H*W,3] fp32.  With m = msk * in_hull:
 *     NB_SAMPLE_H36M   body: m == 1;  bound: in_hull && m != 100   (:160-161,181,190)
 *     NB_SAMPLE_PLAIN  body: m != 0;  bound: in_hull               (:79,99,108)
 *   Candidates of a class are numbered in row-major order (np.argwhere) by an exclusive scan, recomputed on every call.
 *   u dev [n_rounds, n_rays] fp32 uniforms in [0,1).  Round r with deficit m_r (m_0 = n_rays): n_body = (int)(m_r * body_ratio)
 *     body draws, then m_r - n_body bound draws; draw j takes candidate min((int)((double)u[r,j] * count), count - 1).
 *     The pixel's ray, the hit test and near/far are float64 (the reference hands get_near_far the float64 rays here; the
 *     1e-5 / 1e-10 clamps in that order); rays with near < far are appended behind the earlier rounds' in draw order and
 *     m_{r+1} = m_r - hits; it stops at m_r = 0 or after n_rounds rounds.  A class without candidates gives no hits.
 *   outputs dev: rgb, ray_o, ray_d [n_rays,3]; near, far [n_rays] (rounded to fp32 once, on store); pixel [n_rays,2] int32
 *     (y, x); mask_at_box [n_rays] uint8; status [4] int32 = {n_filled, rounds_used, count_body, count_bound}.
 *     Rows >= n_filled: mask_at_box = 0, rgb = 0, pixel = (-1,-1), the ray of pixel (0,0) with near = far = 0.
 *   No synchronisation, no atomics, no data-dependent launch: the same inputs give the same bits.
 *   scratch dev: nb_train_rays_scratch_size(H, W) bytes (0 for sizes the call refuses: H, W < 1 or H*W > 2^30). */
#define NB_SAMPLE_H36M 0
#define NB_SAMPLE_PLAIN 1
int64_t nb_train_rays_scratch_size(int32_t H, int32_t W);
int nb_train_rays(int32_t H, int32_t W, const double K[9], const double R[9], const double T[3], const float bounds[6],
                  const int32_t *hull_xy, int32_t n_hull, const uint8_t *msk, const float *img, int32_t mode,
                  double body_ratio, const float *u, int32_t n_rounds, int32_t n_rays, float *rgb, float *ray_o,
                  float *ray_d, float *near, float *far, int32_t *pixel, uint8_t *mask_at_box, int32_t *status,
                  void *scratch, void *stream);

/* ---------------------------------------------------------------------------------
 * nb_image_assemble — replaces the image re-assembly of the demo visualizer
 * (lib/visualizers/if_nerf_demo.py:15-30; same scatter in lib/evaluators/if_nerf.py:59-68):
 *   img = white_bkgd ? 1 : 0;  img[mask_at_box] = rgb_map;  (optionally) img = img[..., ::-1];  img *= scale
 *   depth = 0;  depth[mask_at_box] = depth_map
 * on device, so a view leaves the GPU (or enters the all-gather) as a finished image.
 *   mask_at_box dev [n_pixels] uint8; rgb_map dev [n_rays,3], depth_map dev [n_rays] or NULL — the
 *   compacted per-ray outputs in pixel order (what nb_raygen + nb_march produce); img dev [n_pixels,3];
 *   depth dev [n_pixels] or NULL (iff depth_map is NULL); scratch dev nb_scan_scratch_size(n_pixels) bytes.
 *   Pixels whose compacted index is >= n_rays keep the background. */
int nb_image_assemble(const uint8_t *mask_at_box, int64_t n_pixels, const float *rgb_map, const float *depth_map,
                      int64_t n_rays, int white_bkgd, int bgr, float scale, float *img, float *depth, void *scratch,
                      void *stream);

/* ---------------------------------------------------------------------------------
 * nb_eval_metrics — replaces Evaluator.evaluate of the quality protocol (lib/evaluators/if_nerf.py:47-74: the scatter
 * at mask_at_box :56-59, mse :65, psnr_metric :15-18) and ssim_metric (:20-45: crop to cv2.boundingRect(mask), then
 * skimage.measure.compare_ssim(multichannel=True) of scikit-image 0.14.2, requirements.txt:6) for one view, on device:
 *   mse   mean (pred - gt)^2 over the compacted fp32 rays (differences and squares in fp32, as the reference's arrays; fp64 sum);
 *         whole_img != 0 (cfg.eval_whole_img): over the whole float64 images, background included
 *   psnr  -10 log10(mse)  (+inf for mse = 0)
 *   ssim  per channel, 7 x 7 uniform window, sample covariance, K1 = 0.01, K2 = 0.03 and compare_ssim's data_range = 2 for
 *         float images; the mean over every window that lies fully inside the crop (the tight box of the non-zero mask
 *         pixels; the whole image with whole_img), then over the 3 channels.  Moments, S and all sums in fp64.
 *   mask_at_box dev [H*W] uint8; rgb_pred, rgb_gt dev [n_rays,3] in compacted pixel order (NULL allowed for n_rays = 0).
 *   Pixels with a zero mask or a compacted index >= n_rays take the background (white_bkgd ? 1 : 0); no image is written.
 *   out dev [8] fp64 = {mse, psnr, ssim, x, y, w, h, n_windows} (x, y, w, h: the crop box, 0,0,0,0 for an empty mask).
 *   A crop under 7 pixels on a side (where compare_ssim raises) gives ssim = NaN and n_windows = 0; n_rays = 0 without
 *   whole_img gives mse = NaN.  Fixed summation order, no floating-point atomics: the same input gives the same bits.
 *   scratch dev: nb_eval_metrics_scratch_size(H, W) bytes (0 for sizes the call refuses: H, W < 1 or H*W > 2^30). */
int64_t nb_eval_metrics_scratch_size(int32_t H, int32_t W);
int nb_eval_metrics(const uint8_t *mask_at_box, int32_t H, int32_t W, const float *rgb_pred, const float *rgb_gt,
                    int64_t n_rays, int white_bkgd, int whole_img, double *out, void *scratch, void *stream);

/* ---------------------------------------------------------------------------------
 * nb_marching_cubes — replaces the mesh extraction of lib/networks/renderer/if_mesh_renderer.py:46-52
 * (mcubes.marching_cubes(cube, cfg.mesh_th) on the host float64 cube) on device, on the fp32 cube itself.
 *   cube dev [X,Y,Z] fp32, C-contiguous (RendererMesh.density_cube); dims = {X, Y, Z}; iso: the threshold (cfg.mesh_th).
 *   A lattice point is inside iff value > iso (equal and NaN are outside).  Case table: csrc/nb_mc_table.h, generated by
 *   tools/gen_mc_table.py (ambiguous faces decided by the face's four signs alone: no cracks; normals point from inside
 *   to outside).  Triangle order and ambiguous-case topology are this table's, not PyMCubes'.
 *   vertices dev [n_vertices,3] fp32 in lattice index units (like PyMCubes): one per lattice edge whose end points differ in
 *   inside-ness, at p0 + t * axis with t = (iso - v0) / (v1 - v0) evaluated in fp64 and the coordinate rounded once to fp32.
 *   Order (part of the contract; no atomics, the same input gives the same bits): vertices by (linear C-order index of the
 *   edge's lower end point, axis 0/1/2); triangles dev [n_triangles,3] int32 vertex indices by (linear C-order index of the
 *   cell's lower point, place in the table row), corners in table order.
 *   nb_marching_cubes_count: flags + two exclusive scans; counts dev [2] = {n_vertices, n_triangles}; no synchronisation.
 *   nb_marching_cubes_emit: same cube, dims, iso and scratch as the count call before it.  Reads the two totals back from the
 *   scratch (8 bytes, one stream synchronisation) and returns NB_EINVAL, writing nothing, when they exceed vert_cap / tri_cap.
 *   scratch dev: nb_marching_cubes_scratch_size(dims) bytes; 0 for dims both calls refuse: a side < 2 or 3*X*Y*Z > 2^31 - 1. */
int64_t nb_marching_cubes_scratch_size(const int32_t dims[3]);
int nb_marching_cubes_count(const float *cube, const int32_t dims[3], float iso, int32_t *counts, void *scratch, void *stream);
int nb_marching_cubes_emit(const float *cube, const int32_t dims[3], float iso, float *vertices, int32_t *triangles,
                           int32_t vert_cap, int32_t tri_cap, void *scratch, void *stream);

/* ---------------------------------------------------------------------------------
 * The query lattice of the mesh pass on device — replaces the per-item host work of
 * lib/datasets/light_stage/multi_view_mesh_dataset.py (get_mask :102-115, prepare_inside_pts :117-140, the meshgrid of
 * __getitem__ :150-158) and the boolean indexing around calculate_density in lib/networks/renderer/if_mesh_renderer.py:30-46.
 *   A lattice is three DEVICE fp32 axis vectors ax [X], ay [Y], az [Z] and dims = {X, Y, Z} (host): point (i, j, k) =
 *   (ax[i], ay[j], az[k]), linear index (i*Y + j)*Z + k — np.meshgrid(x, y, z, indexing='ij') (:157) without the [X,Y,Z,3]
 *   array.  Every side >= 1, X*Y*Z <= 2^31 - 1, else NB_EINVAL.  scratch dev: nb_scan_scratch_size(X*Y*Z) bytes.
 *   No atomics, no synchronisation: the same inputs give the same bits.
 * nb_mask_dilate — cv2.dilate(msk, np.ones((border, border), np.uint8)) of get_mask (:111-113) for n_views masks at once:
 *   out[v,y,x] = max of msk[v] over the border x border window centred on (y, x); pixels outside the image are ignored
 *   (cv2's default border value for dilation); border odd, 1..255 (1 copies).  msk, out dev [n_views,H,W] uint8, distinct.
 * nb_lattice_carve — prepare_inside_pts (:117-140): inside[p] = 1 iff point p projects onto a non-zero pixel of every view's
 *   mask, else 0.  The projection, the rounding (half to even), the clamp to the image and the treatment of non-finite pixel
 *   coordinates are those of nb_cull in nb_march (one device function serves both); cull->pre_affine must be 0.
 *   cull HOST pointer, its members DEVICE pointers; inside dev [X*Y*Z] uint8 out; n_inside dev [1] int32 out = the flag sum.
 * nb_lattice_gather — pts[inside] (if_mesh_renderer.py:30-31) of ANY bitmap (non-zero = flagged), in linear order:
 *   wpts dev [cap,3] fp32 = the flagged points' coordinates (the axis values, bit for bit), lin dev [cap] int32 = their linear
 *   indices (np.flatnonzero(inside)); flagged points beyond cap are dropped and nothing is written behind row min(total, cap);
 *   n_out dev [2] int32 = {min(total, cap), total}.  cap = 0 only counts (wpts, lin may be NULL).
 * nb_lattice_scatter — cube[inside] = alpha; np.pad(cube, pad) (if_mesh_renderer.py:42-46) in one step: cube dev
 *   [X+2*pad, Y+2*pad, Z+2*pad] fp32, ZEROED BY THE CALLER; cube[i+pad, j+pad, k+pad] = alpha[r * alpha_stride] for the point
 *   (i, j, k) = lin[r], r < n (n <= X*Y*Z; an entry of lin that is no lattice point writes nothing).  alpha_stride in floats:
 *   1 for the [1,n,1] tensor of calculate_density. */
int nb_mask_dilate(const uint8_t *msk, int32_t n_views, int32_t H, int32_t W, int32_t border, uint8_t *out, void *stream);
int nb_lattice_carve(const float *ax, const float *ay, const float *az, const int32_t dims[3], const nb_cull *cull,
                     uint8_t *inside, int32_t *n_inside, void *scratch, void *stream);
int nb_lattice_gather(const float *ax, const float *ay, const float *az, const int32_t dims[3], const uint8_t *inside,
                      int32_t cap, float *wpts, int32_t *lin, int32_t *n_out, void *scratch, void *stream);
int nb_lattice_scatter(const float *alpha, int64_t alpha_stride, const int32_t *lin, int64_t n, const int32_t dims[3],
                       int32_t pad, float *cube, void *stream);

/* ---------------------------------------------------------------------------------
 * A frame's geometry from SMPL parameters on device — replaces the offline vertex export of zju_smpl/extract_vertices.py
 * (SMPLlayer.forward, zju_smpl/smplmodel/body_model.py:89-153, over lbs, zju_smpl/smplmodel/lbs.py:142-233, 280-378) and the
 * per-frame prepare_input of lib/datasets/light_stage/multi_view_dataset.py:68-118 / monocular_dataset.py:32-71.
 *   Plain fp32, no atomics, no allocation, no synchronisation: the same inputs give the same bits.
 * nb_smpl_model — HOST struct, its arrays DEVICE fp32, laid out for the kernels (neuralbody_amd/smpl_pose.py::SmplModel):
 *   v_template [3V]; shapedirs [10, 3V] (basis-major); posedirs [207, 3V] (the reference's own reshape, body_model.py:51; may be
 *   NULL when new_params is never set); weights [24, V] (joint-major); j_template [24,3] = J_regressor . v_template and
 *   j_shapedirs [24,3,10] = J_regressor . shapedirs, regressed once on the host; parents HOST [24], parents[0] = -1 and
 *   0 <= parents[j] < j otherwise, else NB_EINVAL.
 * nb_smpl_pose — params dev [F, NB_SMPL_PARAMS] fp32, one row per frame: poses 72 | shapes 10 | Rh 3 | Th 3 (the keys of
 *   EasyMocap's params/{i}.npy).  verts dev [F,V,3] out: the world vertices body_model.py:148 returns (scale = 1); joints dev
 *   [F,24,3] out or NULL: the posed joints (lbs.py:371) in the body's own frame.  new_params != 0 adds the pose blend shapes
 *   (lbs.py:210-213); with 0 posedirs is never read.  batch_rodrigues is restated as written (angle = |r + 1e-8|, direction
 *   r / angle, lbs.py:295-296).  Two sums are arranged so that the rest pose returns the shaped body exactly: the relative
 *   transform's translation is accumulated along the chain as A_parent.t + G_parent.R (I - R_j) J_j (lbs.py:375-376 subtracts two
 *   joint-sized numbers), and the blend is [I|0] + sum_j W[v,j] (A_j - [I|0]), which equals sum_j W[v,j] A_j (lbs.py:223) for
 *   weights that sum to 1 per vertex.  ws dev [F, NB_SMPL_WS_FLOATS] fp32 scratch.  Two launches: one wave per frame (rotations,
 *   joints, chain), then 64 vertices per workgroup, which reads every element of posedirs once per frame.
 *   1 <= F <= 65535, V >= 1, else NB_EINVAL.
 * nb_smpl_voxelize — prepare_input for verts dev [F,V,3] already on the device, one workgroup per frame.  Rh, Th dev: frame f's
 *   three floats at Rh + f * rt_stride, Th + f * rt_stride (rt_stride in floats, >= 3: 3 for [F,3] arrays, NB_SMPL_PARAMS for the
 *   columns of params).  voxel_size HOST [3] doubles in dhw order, each > 0 (cfg.voxel_size as Python floats).
 *   pad_mode: NB_PAD_ZJU z -+ 0.05 (multi_view_dataset.py:80-81), NB_PAD_BIG_BOX all axes -+ 0.05 (:76-78), NB_PAD_SNAPSHOT
 *   y -+ 0.1 (monocular_dataset.py:38-39), a float32 subtraction as numpy's on a float32 array; anything else NB_EINVAL.
 *   R dev [F,3,3] out: cv2.Rodrigues(Rh) evaluated in double and rounded to fp32 (NOT the fp32 formula of the skinning step).
 *   bounds dev [F,2,3] out: padded min / max of (v - Th) . R in fp32.  coord dev [F,V,3] int32 out, dhw order:
 *   int32(rint(double(dhw - min_dhw) / voxel_size)), the subtraction in fp32, rounding half to even (np.round, :111).
 *   out_sh dev [F,3] int32 out: (int32(ceil(double(max_dhw - min_dhw) / voxel_size)) | 31) + 1 (:114-116).
 *   summary dev [F,9] int32 out: the six fp32 of can_bounds (padded min / max of the world vertices, :73-83) bit-cast, then
 *   out_sh — everything the host needs of a frame, in one 36-byte copy. */
#define NB_SMPL_JOINTS 24
#define NB_SMPL_POSE_BASIS 207
#define NB_SMPL_BETAS 10
#define NB_SMPL_PARAMS 88
#define NB_SMPL_WS_FLOATS 512
#define NB_PAD_ZJU 0
#define NB_PAD_BIG_BOX 1
#define NB_PAD_SNAPSHOT 2
typedef struct nb_smpl_model {
    int32_t n_verts;
    int32_t parents[NB_SMPL_JOINTS];
    const float *v_template, *shapedirs, *posedirs, *weights, *j_template, *j_shapedirs;
} nb_smpl_model;
int nb_smpl_pose(const nb_smpl_model *model, const float *params, int32_t n_frames, int new_params, float *ws, float *verts,
                 float *joints, void *stream);
int nb_smpl_voxelize(const float *verts, int32_t n_verts, int32_t n_frames, const float *Rh, const float *Th, int64_t rt_stride,
                     const double voxel_size[3], int pad_mode, int32_t *coord, int32_t *out_sh, float *bounds, float *R,
                     int32_t *summary, void *stream);

/* ---------------------------------------------------------------------------------
 * nb_smpl_silhouette — cull masks of a pose that was never photographed: the posed body's triangles rasterised into the cull
 * cameras on device.  The reference's novel-pose dataset reads the CIHP masks of real images from disk
 * (lib/datasets/light_stage/multi_view_perform_dataset.py:105-127); the consumer is the sample cull of
 * lib/networks/renderer/if_clight_renderer_mmsk.py:12-45 (nb_cull in nb_march), whose round -> clamp lookup fixes the pixel
 * convention here.  No allocation, no synchronisation; the output is a function of the inputs alone (the same bits every call).
 *   verts dev [F,V,3] fp32 (nb_smpl_pose); faces dev [Nf,3] int32 vertex indices, either winding (a face with an index outside
 *   0..V-1 is skipped; neuralbody_amd/smpl_pose.py::SmplModel validates the list once on the host); cam dev [nv,21] fp32, the
 *   layout of nb_cull.cam (RT 3x4 | K 3x3).  out dev [F,nv,H,W] uint8, 1 = body; a dirty buffer is fine.
 *   Projection: p = R v + T, (u, w) = (K p).xy / (K p).z in fp32, nb_cull's arithmetic (FMA chains, above; one device function serves both).  u, w are snapped to 1/256
 *   pixel (rintf(256 u), half to even) and held as integers.  Pixel (x, y) is the closed unit square centred on the integer
 *   point (x, y).  Coverage is conservative and exact: a pixel is set for a triangle iff its square meets the closed snapped
 *   triangle — the square overlaps the triangle's bounding box and, with the triangle oriented to positive area, every int64
 *   edge function satisfies E_i(pixel centre) + 128 (|dx_i| + |dy_i|) >= 0 (1/256 units).  A snapped triangle of zero area is
 *   skipped.  The mask is the union over the triangles.
 *   A (frame, view) with any vertex at camera depth (R v + T).z < 0.01 m, or projecting beyond +-32768 px (or to a NaN),
 *   does not cull: its mask is all 1.  The other views of the call are unaffected.  (The bound keeps every product below 2^48.)
 *   1 <= F <= 65535, V, Nf >= 1, 1 <= nv <= NB_MAX_CULL_VIEWS, F nv V and F nv Nf < 2^31 - 256, 1 <= H, W <= 32768, else
 *   NB_EINVAL.  scratch dev, 16-byte aligned: nb_smpl_silhouette_scratch_size(F, V, Nf, nv) bytes (0 for refused dimensions).
 *   Five stream operations: a memset of the scratch header, the projection, a fill (0, or 1 for a view that does not cull), one
 *   thread per (frame, view, triangle) that walks a clipped bounding box of at most 16 x 16 pixels, and a fixed grid that gives
 *   each larger triangle a workgroup (their list and its count stay in the scratch). */
int64_t nb_smpl_silhouette_scratch_size(int32_t n_frames, int32_t n_verts, int32_t n_faces, int32_t n_views);
int nb_smpl_silhouette(const float *verts, const int32_t *faces, const float *cam, int32_t n_frames, int32_t n_verts,
                       int32_t n_faces, int32_t n_views, int32_t H, int32_t W, void *scratch, int64_t scratch_bytes, uint8_t *out,
                       void *stream);

/* ---------------------------------------------------------------------------------
 * Pictures of an extracted mesh on device — replaces the OpenGL renderer behind tools/render_mesh.py (tools/render/*: pyglet,
 * PyOpenGL, GLSL) for the one thing the mesh workflow uses it for: orthographic, z-buffered, normal-shaded views.  No allocation,
 * no synchronisation, everything on `stream`; every output is a function of the inputs alone (the same bits every call).
 * "a (+) b" below is ONE fp32 operation rounded to nearest; no two are contracted into an FMA.
 * nb_mesh_vertex_normals — compute_normal and normalize_v3 (tools/render_mesh.py:21-51).  verts dev [V,3] fp32, faces dev [T,3]
 *   int32 (a face with an index outside 0..V-1 is skipped), acc dev [V,3] int32 scratch (zeroed here; a dirty buffer is fine),
 *   normals dev [V,3] fp32 out.  Face normal: u = b (-) a, w = c (-) a, n = (u.y (*) w.z (-) u.z (*) w.y, ...), len =
 *   max(sqrt((n.x (*) n.x (+) n.y (*) n.y) (+) n.z (*) n.z), 1e-8f), q = rint((n (/) len) (*) 2^20) as int32, added to the three
 *   vertices' sums with integer atomics: the sums do not depend on arrival order.  |q| <= 2^20 + 1, so a vertex of valence up to
 *   2047 cannot overflow (2047 (2^20 + 1) < 2^31).  A face whose q is not finite adds nothing.  Vertex normal: s = float(sum) (*)
 *   2^-20, s (/) max(|s| as above, 1e-8f); a vertex used by no face gets (0, 0, 0).  0 <= V <= (2^31 - 257) / 3, 0 <= T <=
 *   2^31 - 257, else NB_EINVAL.  A memset and two launches (a thread per face, a thread per vertex).
 * nb_mesh_render — set_mesh / display / get_color of tools/render_mesh.py:146-167 for n_views cameras at once (color_render.py,
 *   color.vs, color.fs; GL_LESS, no culling, no multisampling, white clear colour).  normals dev [V,3] fp32 (the call above);
 *   cams dev [n_views, NB_MESH_CAM_FLOATS] fp32, per view: M 3x4 row-major, (x_px, y_px, d) = M . (v, 1) with row r evaluated as
 *   ((M_r0 (*) v.x (+) M_r1 (*) v.y) (+) M_r2 (*) v.z) (+) M_r3 | N 3x3 row-major, the rotation of the normals, each row the same
 *   three-term sum | 3 floats of padding (neuralbody_amd/mesh_render.py::turntable_cams composes both in float64).  Pixel (i, j)
 *   (column, row) is sampled at (i + 1/2, j + 1/2); the smaller d is nearer.
 *   Outputs: rgb dev [n_views,H,W,3] fp32; face_id dev [n_views,H,W] int32 or NULL; depth dev [n_views,H,W] fp32 or NULL.
 *   Background is (1,1,1), -1, +inf; the whole of every output is written, so a dirty buffer is fine.
 *   x_px, y_px are snapped to 1/256 pixel (rintf(256 x), half to even) and held as integers; the triangle is oriented to
 *   positive area by exchanging its second and third vertex, attributes included.  Skipped: a face with an index outside
 *   0..V-1, a non-finite x_px, y_px or d, |x_px| or |y_px| > 32768, zero snapped area.  Coverage is exact: with
 *   E_i = the int64 edge function of the edge opposite vertex i at (256 i + 128, 256 j + 128), the pixel is covered iff
 *   E_0, E_1, E_2 >= 0 (closed triangles, both windings).  l_i = float(E_i) (/) float(E_0 + E_1 + E_2); an attribute is
 *   (a_0 (+) l_1 (*) (a_1 (-) a_0)) (+) l_2 (*) (a_2 (-) a_0): d, and each channel of the vertex colour 0.5 (*) (N . n) (+) 0.5.  A
 *   sample whose d is not finite is not drawn.  The pixel keeps the sample with the smallest key = (bits of d, order-preserving,
 *   -0 below +0) << 32 | triangle index: the smallest depth, a tie going to the lower triangle.
 *   n_views >= 1, 1 <= H, W <= 32768, T >= 0 (T = 0: background), n_views H W and n_views T < 2^31 - 256, else NB_EINVAL.
 *   scratch dev, 16-byte aligned: nb_mesh_render_scratch_size(n_views, H, W, T) bytes (0 for refused dimensions): a header, the
 *   [n_views,H,W] uint64 keys, the list of large triangles.
 *   Five stream operations: two memsets (the header; the keys to all ones), a thread per (view, triangle) that projects its three
 *   vertices itself, walks a clipped box of at most 16 x 16 pixel centres and issues one 64-bit atomicMin per covered centre
 *   (after a plain read of the key that may skip it), a fixed grid that gives each larger triangle a workgroup, and a thread per
 *   pixel that decodes the winner, repeats its projection by the same function and interpolates the colour. */
#define NB_MESH_CAM_FLOATS 24
int nb_mesh_vertex_normals(const float *verts, const int32_t *faces, int32_t n_verts, int32_t n_faces, int32_t *acc,
                           float *normals, void *stream);
int64_t nb_mesh_render_scratch_size(int32_t n_views, int32_t H, int32_t W, int32_t n_faces);
int nb_mesh_render(const float *verts, const float *normals, const int32_t *faces, int32_t n_verts, int32_t n_faces,
                   const float *cams, int32_t n_views, int32_t H, int32_t W, float *rgb, int32_t *face_id, float *depth,
                   void *scratch, int64_t scratch_bytes, void *stream);

/* ---------------------------------------------------------------------------------
 * The extracted mesh cleaned and coloured on device — the reference has neither: every stray blob of density above cfg.mesh_th
 * becomes a closed surface of its own in the .ply (lib/networks/renderer/if_mesh_renderer.py:46-52, lib/visualizers/
 * if_nerf_mesh.py:26-34) and the mesh is grey.  The host equivalent of the first three calls is a download,
 * scipy.sparse.csgraph.connected_components, numpy indexing and an upload.
 *   Rules of every call: no allocation, no synchronisation, everything on `stream`; integer atomics only, and only where the
 *   result does not depend on arrival order, so the same input gives the same bits; every loop is counted and no thread waits for
 *   another; a loop that reaches its limit sets the GIVE-UP WORD, the first int32 of the scratch, and the thread leaves.
 *   faces dev [T,3] int32; a face with an index outside 0..V-1 is skipped (the rule of nb_mesh_vertex_normals): it connects
 *   nothing, counts for no component and does not survive the compaction.  0 <= V, T <= 2^31 - 257, else NB_EINVAL.
 *   scratch dev, 16-byte aligned: nb_mesh_clean_scratch_size(V, T) bytes (0 for refused sizes).  ONE scratch serves the calls of
 *   one mesh, in this order: components writes the give-up word, select and compact_count read it; compact_count leaves the scan
 *   positions that compact reads.  A caller with labels or flags of its own zeroes the first 4 bytes instead.
 * nb_mesh_components — label dev [V] int32 out: the smallest vertex index of v's connected component, two vertices being
 *   connected when a face uses both; a vertex no face uses is its own component.  Union-find in the scratch under the invariant
 *   parent[v] <= v: a thread per face unites (a, b) and (a, c), hooking the larger root under the smaller with atomicMin; when
 *   the atomicMin returns another value than the root it expected, the thread goes on with the pair (returned value, smaller
 *   root), whose larger member has strictly decreased.  The root of a set is therefore its minimum whatever the order of the
 *   hooks.  Paths are halved on the way (parent[v] = min(parent[v], grandparent), atomicMin again).  A face spends at most 2^14
 *   parent reads and hook attempts; if one runs out, the hook launch (idempotent) runs again, up to NB_MESH_HOOK_ROUNDS launches
 *   in all, every launch after the first returning at once unless the one before it gave up (a word per round in the scratch
 *   header: nothing is read back).  Then a thread per vertex walks to its root (at most 2^20 steps).  If the last round or a
 *   walk gave up, the give-up word is 1 and label is NOT written; else it is 0.
 * nb_mesh_component_select — which components stay.  label as above.  The faces of a component are counted at its label
 *   (atomicAdd); the largest count wins, a tie going to the smaller label (one 64-bit atomicMax of count << 32 | ~label).
 *   keep_vertex dev [V] uint8 out: min_fraction = 1: 1 iff v lies in the winning component ("largest": exactly one component);
 *   0 < min_fraction < 1: 1 iff its component's face count >= max(1, ceil(double(min_fraction) * largest count)).  A component
 *   without a face is never kept.  stats dev [4] int32 out = {components that have a face, components kept, faces of the
 *   largest, faces kept}.  With the give-up word set: keep_vertex is not written and stats = {NB_EINTERNAL x 4}.
 * nb_mesh_compact_count / nb_mesh_compact — the kept part as a mesh of its own.  keep_vertex dev [V] uint8 (any flags, non-zero
 *   = kept).  A face is kept iff its three indices are in range and its FIRST vertex is kept (with the flags of the call above
 *   its other two are then kept as well; with other flags an index of a dropped vertex becomes -1).  Two exclusive scans (the
 *   tile body of csrc/nb_scan_dev.h) number the kept vertices and the kept faces, so both keep their relative order: the
 *   order contract of nb_marching_cubes holds for the result as a subsequence.  counts dev [2] int32 out = {kept vertices, kept
 *   faces}, or {NB_EINTERNAL, NB_EINTERNAL} with the give-up word set.  The caller reads these 8 bytes to size the outputs (the
 *   capacity rule of nb_marching_cubes_emit) and reports NB_EINTERNAL when it finds it there.
 *   nb_mesh_compact, after nb_mesh_compact_count with the same faces, flags and scratch: verts dev [V,3] fp32 -> verts_out dev
 *   [vert_cap,3]; faces -> faces_out dev [tri_cap,3] int32, indices renumbered; attr dev [V,3] fp32 or NULL (normals, colours)
 *   -> attr_out dev [vert_cap,3] or NULL, each row with its vertex.  Rows behind the counts are left alone.  With the give-up
 *   word set, or a count above its capacity, NOTHING is written (tested on the device; the caller compares the counts it read).
 * nb_mesh_color_query — what the colour head is asked at every vertex.  verts_idx dev [V,3] fp32 in index units of the padded
 *   cube (nb_marching_cubes), normals dev [V,3] fp32 (nb_mesh_vertex_normals of the WORLD vertices), step, origin dev [3] fp32,
 *   pad: wpts dev [V,3] out = ((v (-) pad) (*) step) (+) origin per axis, three fp32 operations, none contracted (RendererMesh's
 *   world=True); viewdir dev [V,3] out = -n: looking straight at the surface from outside (the table's normals point outwards).
 *   A zero normal (a vertex no face uses) gives (0, 0, -1).
 * nb_mesh_color_finish — raw dev [V,4] fp32 (calculate_density_color: rgb logits, sigma) -> rgb_f dev [V,3] fp32 =
 *   1 (/) (1 (+) expf(-raw)), the sigmoid as nb_composite evaluates it; rgb_u8 dev [V,3] uint8 = rint(255 (*) rgb_f), half to
 *   even, clamped to 0..255 (a NaN gives 0).
 * nb_mesh_render_attr — nb_mesh_render with the vertex colour READ from attr dev [V,3] fp32 instead of computed as
 *   0.5 (*) (N . n) (+) 0.5: the same cameras, snapped coverage, 64-bit key and interpolation expression (one triangle walker,
 *   one resolve kernel in two instantiations).  Fed that expression as attr, it returns nb_mesh_render's bits.  Same scratch. */
#define NB_EINTERNAL (-4) /* a counted device loop gave up (written into device outputs; see the mesh clean-up) */
#define NB_MESH_HOOK_ROUNDS 4
int64_t nb_mesh_clean_scratch_size(int32_t n_verts, int32_t n_faces);
int nb_mesh_components(const int32_t *faces, int32_t n_verts, int32_t n_faces, int32_t *label, void *scratch, void *stream);
int nb_mesh_component_select(const int32_t *label, const int32_t *faces, int32_t n_verts, int32_t n_faces, float min_fraction,
                             uint8_t *keep_vertex, int32_t *stats, void *scratch, void *stream);
int nb_mesh_compact_count(const int32_t *faces, const uint8_t *keep_vertex, int32_t n_verts, int32_t n_faces, int32_t *counts,
                          void *scratch, void *stream);
int nb_mesh_compact(const float *verts, const int32_t *faces, const float *attr, int32_t n_verts, int32_t n_faces,
                    float *verts_out, int32_t *faces_out, float *attr_out, int32_t vert_cap, int32_t tri_cap, void *scratch,
                    void *stream);
int nb_mesh_color_query(const float *verts_idx, const float *normals, const float *step, const float *origin, float pad,
                        int32_t n_verts, float *wpts, float *viewdir, void *stream);
int nb_mesh_color_finish(const float *raw, int32_t n_verts, float *rgb_f, uint8_t *rgb_u8, void *stream);
int nb_mesh_render_attr(const float *verts, const float *attr, const int32_t *faces, int32_t n_verts, int32_t n_faces,
                        const float *cams, int32_t n_views, int32_t H, int32_t W, float *rgb, int32_t *face_id, float *depth,
                        void *scratch, int64_t scratch_bytes, void *stream);

/* ---------------------------------------------------------------------------------
 * Field normals on device — the surface normal of the density field, n(p) = -grad sigma(p) / |grad sigma(p)|, for the samples of
 * a marched view and for mesh vertices.  replaces: nothing in the reference (it has no normal output; its turntable shades with
 * the face normals of the marching-cubes mesh, tools/render_mesh.py:21-51).  The decoder part of d sigma / dp is the tap of
 * nb_decode_points and three nb_gemm_fused products (Network.calculate_density_gradient); these calls are the rest.
 *   Rules of every call: no allocation, no synchronisation, no atomics, everything on `stream`: the same inputs give the same
 *   bits.  n == 0 (no point, no sample, no ray) returns NB_OK at once and looks at no pointer.
 * nb_trilinear_grad — replaces: nothing in the reference.  The coordinate twin of nb_trilinear_bwd: the same scene, the same
 *   index grids, and rows[l] dev [n_rows_l, C_l] fp32, 16-byte aligned: the ACTIVE rows of level l (scene->vol[] is not read).
 *   wpts dev [n,3] world points, d_feat dev [n,352] (16-byte aligned) -> grad dev [n,3] out, world axes; 0 <= n < 2^31 - 256, else NB_EINVAL:
 *       grad[p] = d/dp ( sum_c d_feat[p,c] F_c(p) ),  F the 4-level lookup of latent_xyzc.py:62-72.
 *   Per level l of size (D, H, W): the index coordinates (ix, iy, iz), the cell (x0, y0, z0) = their floors and the weight pairs
 *   wx = {x0 + 1 - ix, ix - x0}, wy, wz are the forward gather's, formed by the same device functions; v(dx,dy,dz)[c] is the row
 *   the grid names for voxel (x0+dx, y0+dy, z0+dz), or 0 for a voxel out of bounds or with grid entry -1.
 *       t_x = sum_c d_feat[c] sum_{dy,dz} wy[dy] wz[dz] (v(1,dy,dz)[c] - v(0,dy,dz)[c]),   t_y, t_z alike
 *   (evaluated as sum_{dy,dz} wy wz (p(1,dy,dz) - p(0,dy,dz)) with p(corner) = sum_c d_feat[c] v(corner)[c]).  The gradient of a
 *   point is that of the cell the forward assigns it: at an integer index coordinate the right-hand derivative.  A level whose
 *   index coordinate was clamped (outside [-2, size + 1]) contributes 0.  Canonical gradient gc_x = sum_l t_x,l (W_l - 1) /
 *   (voxel_size[2] out_sh[2]), gc_y with H_l and [1], gc_z with D_l and [0]; world gradient grad_i = sum_j R[i][j] gc_j (canonical
 *   = (p - Th) @ R).  fp32 throughout.  Eight lanes serve a point (each 16-byte piece of a row is read once), a wave eight
 *   consecutive points.
 * nb_normal_select — replaces: nothing in the reference.  Which samples of a marched view get a gradient: every (ray, s) with
 *   weights[ray, s] >= w_min (a NaN is not selected), in (ray, s) order.  ray_o, ray_d dev [n_rays,3], near, far dev [n_rays],
 *   t_vals dev [S], t_rand dev [n_rays,S] or NULL, weights dev [n_rays,S] (nb_march's output): the arguments of that march.
 *   idx dev [cap] int32 out = ray * S + s; wpts dev [cap,3] fp32 out = the sample's position by the march's own steps (z_lin,
 *   the stratified jitter when t_rand is given, ray_point: bit for bit the point the march decoded); selected samples beyond
 *   cap are dropped and nothing is written behind row min(total, cap); n_out dev [2] int32 = {min(total, cap), total}.  cap = 0
 *   only counts (idx, wpts may be NULL): the caller reads these 8 bytes to size the outputs, the capacity rule of
 *   nb_lattice_gather.  n_rays * S < 2^31 - 256, else NB_EINVAL.  scratch dev: nb_scan_scratch_size(n_rays * S) bytes.
 * nb_normal_composite — replaces: nothing in the reference.  idx dev [m] int32 ascending (nb_normal_select's), grad dev [m,3]
 *   fp32 (d sigma / dp of the selected samples), weights dev [n_rays,S] -> normal_map dev [n_rays,3], normal_acc dev [n_rays],
 *   EVERY ray written.  Per selected sample nhat = -grad (/) |grad|, or 0 when |grad| < 1e-12 or not finite (|grad| =
 *   sqrt((gx gx (+) gy gy) (+) gz gz) in fp32).  Per ray, over its selected samples in sample order, one IEEE operation per step,
 *   none contracted: sum = sum (+) w_s (*) nhat_s per axis, normal_acc = sum_s w_s (every selected sample, also one without a
 *   direction); normal_map = sum (/) |sum|, or (0, 0, 0) when |sum| < 1e-6 or not finite.  A thread per ray finds its run in idx
 *   by bisection.  0 <= m <= n_rays * S < 2^31 - 256, else NB_EINVAL. */
int nb_trilinear_grad(const nb_scene *scene, const int32_t *const grids[4], const float *const rows[4], const float *wpts,
                      const float *d_feat, int64_t n, float *grad, void *stream);
int nb_normal_select(const float *ray_o, const float *ray_d, const float *near, const float *far, int64_t n_rays, int32_t n_samples,
                     const float *t_vals, const float *t_rand, const float *weights, float w_min, int32_t cap, int32_t *idx,
                     float *wpts, int32_t *n_out, void *scratch, void *stream);
int nb_normal_composite(const int32_t *idx, const float *grad, int64_t m, const float *weights, int64_t n_rays, int32_t n_samples,
                        float *normal_map, float *normal_acc, void *stream);

/* ---------------------------------------------------------------------------------
 * A photographed frame on device — replaces the OpenCV calls between the image files and the kernels above:
 * lib/datasets/light_stage/multi_view_dataset.py:58-64 (get_mask: cv2.erode, cv2.dilate, the border band), :129-142 (cv2.undistort
 * of the float32 image and the uint8 mask, cv2.resize INTER_AREA / INTER_NEAREST by cfg.ratio, the background fill) and
 * lib/datasets/light_stage/multi_view_mesh_dataset.py:102-109 (cv2.undistort of every view's mask).  The inputs are the files'
 * BYTES (3 per pixel and 1 per pixel); no float image of the full resolution is ever written.  No allocation, no
 * synchronisation, no atomics, everything on `stream`: the same inputs give the same bits.  "a (+) b" below is ONE IEEE operation
 * rounded to nearest; no two are contracted into an FMA.
 * nb_mask_band — get_mask (:58-64) for n_views label images at once, in one pass (no eroded or dilated image is written).
 *   label, out dev [n_views,H,W] uint8, distinct.  m = (label != 0); e, d = the minimum and the maximum of m over the
 *   border x border window centred on the pixel, pixels outside the image ignored (cv2's default border for both: the rule of
 *   nb_mask_dilate); out = 100 where d - e == 1, else m.  border odd, 1..255; border = 1 gives m.
 * nb_image_undistort — cv2.undistort(src, K, D) with newCameraMatrix = K (:129-130; mesh dataset :109), then the reduction by
 *   the integer factor n = 1 / cfg.ratio (:136-138) and the fill (:139-142), for n_views views with a camera each.
 *   rgb dev [n_views,H,W,3] uint8 or NULL; msk dev [n_views,H,W] uint8 or NULL (not both NULL); img_out dev
 *   [n_views,H/n,W/n,3] fp32, NULL iff rgb is; msk_out dev [n_views,H/n,W/n] uint8, NULL iff msk is.
 *   cam HOST [n_views, NB_CAM_DOUBLES] float64: fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 (a 4-entry D has k3 = 0, a 4- or 5-entry D
 *   k4 = k5 = k6 = 0), every entry finite, fx and fy non-zero.
 *   Source position of full-resolution pixel (column j, row i), in float64, in this order:
 *     x = (j (-) cx) (/) fx;  y = (i (-) cy) (/) fy;  x2 = x (*) x;  y2 = y (*) y;  r2 = x2 (+) y2;  _2xy = (2 (*) x) (*) y
 *     kr = (1 (+) ((k3 (*) r2 (+) k2) (*) r2 (+) k1) (*) r2) (/) (1 (+) ((k6 (*) r2 (+) k5) (*) r2 (+) k4) (*) r2)
 *     u = fx (*) ((x (*) kr (+) p1 (*) _2xy) (+) p2 (*) (r2 (+) 2 (*) x2)) (+) cx
 *     v = fy (*) ((y (*) kr (+) p1 (*) (r2 (+) 2 (*) y2)) (+) p2 (*) _2xy) (+) cy
 *   iu = rint(u (*) 32), iv = rint(v (*) 32) (half to even), clamped into int32, a NaN giving -2^31; sx = iu >> 5, sy = iv >> 5,
 *   ax = iu & 31, ay = iv & 31: OpenCV's 1/32-pixel fixed-point map.  The taps are (sy, sx), (sy, sx+1), (sy+1, sx),
 *   (sy+1, sx+1); a tap outside the image reads 0 (BORDER_CONSTANT).
 *   uint8: w00 = (32-ay)(32-ax), w01 = (32-ay) ax, w10 = ay (32-ax), w11 = ay ax; value = (sum S w + 512) >> 10.
 *   float: S = float(byte) (/) 255.f; gx = 1 (-) ax (/) 32.f, fx = ax (/) 32.f, likewise gy, fy; w00 = gy (*) gx, w01 = gy (*) fx,
 *     w10 = fy (*) gx, w11 = fy (*) fx; value = ((S00 (*) w00 (+) S01 (*) w01) (+) S10 (*) w10) (+) S11 (*) w11 in fp32.
 *   Reduction: msk_out(Y, X) = the undistorted mask at (nY, nX) (INTER_NEAREST by an integer factor); img_out(Y, X) = the fp32
 *   sum, from 0 and in row-major order, of the n x n undistorted pixels of block (nY.., nX..), (*) (1.f (/) float(n n))
 *   (INTER_AREA by an integer factor).  n >= 1 divides H and W; n = 1 copies.
 *   fill: NB_FILL_NONE, or NB_FILL_BLACK / NB_FILL_WHITE: img_out = 0 / 1 where msk_out == 0 (needs msk).
 *   n_views >= 1, 1 <= H, W <= 32768, 3 n_views H W <= 2^31 - 1, else NB_EINVAL.  One launch per 8 views, one thread per
 *   output pixel. */
#define NB_CAM_DOUBLES 12
#define NB_FILL_NONE 0
#define NB_FILL_BLACK 1
#define NB_FILL_WHITE 2
int nb_mask_band(const uint8_t *label, int32_t n_views, int32_t H, int32_t W, int32_t border, uint8_t *out, void *stream);
int nb_image_undistort(const uint8_t *rgb, const uint8_t *msk, const double *cam, int32_t n_views, int32_t H, int32_t W, int32_t n,
                       int fill, float *img_out, uint8_t *msk_out, void *stream);

/* ---------------------------------------------------------------------------------
 * An animatable mesh on device — the extracted mesh bound to the SMPL body it clothes, after which it IS an nb_smpl_model with
 * V = its vertex count: nb_smpl_pose reposes it, nb_mesh_vertex_normals / nb_mesh_render(_attr) draw it, nb_smpl_silhouette
 * gives clothed cull masks.  replaces: the inverse skin is ppts_to_pts (lib/utils/blend_utils.py:73-82), which the reference
 * applies to the sample points of its T-pose variant; it has no mesh counterpart.  Plain fp32, "a (+) b" ONE operation rounded
 * to nearest, none contracted; dot(x, y) = (x0 (*) y0 (+) x1 (*) y1) (+) x2 (*) y2.  No allocation, no synchronisation, everything
 * on `stream`; the outputs are a function of the inputs alone (the same bits every call, into a dirty buffer too).
 * nb_mesh_closest — points dev [P,3] fp32, verts dev [V,3] fp32, faces dev [Nf,3] int32 -> face dev [P] int32, bary dev [P,3]
 *   fp32, dist2 dev [P] fp32: for every point the triangle with the smallest squared distance over ALL triangles, the lower face
 *   index on a tie.  A face with an index outside 0..V-1 is skipped (the rule of nb_mesh_vertex_normals), and so is a face whose
 *   dist2 comes out non-finite (collinear corners can divide 0 by 0).  A point with no valid face, or a non-finite point, gets
 *   face = -1, bary = 0, dist2 = +inf.  Per triangle: the region walk of Ericson, Real-Time Collision Detection 5.1.5, with
 *   ab = b (-) a, ac = c (-) a, ap = p (-) a, d1 = dot(ab, ap), d2 = dot(ac, ap), ... the vertex, edge and interior regions tested
 *   in the book's order, edge parameters IEEE divisions (d1 (/) (d1 (-) d3), ...), the interior denom = 1 (/) ((va (+) vb) (+) vc)
 *   with each of va, vb, vc first replaced by 0 where negative (nothing in exact arithmetic; it bounds v and w whatever rounding
 *   did to the region tests), v = vb (*) denom, w = vc (*) denom; then bary = ((1 (-) v) (-) w, v, w), q = (a (+) ab (*) v) (+)
 *   ac (*) w, dist2 = dot(p (-) q, p (-) q).  csrc/nb_mesh_rig.hip writes every line out; tests/mesh_rig_ref.py restates it in
 *   float32 numpy to the bit.  One thread per point (below 1024 workgroups of 64 points, up to 16 waves share the tiles of a
 *   workgroup's points and merge under the same order); a prepass (six small launches) sorts the faces into spatially compact tiles
 *   of 64 with a bounding sphere each, which a wave skips when the sphere's lower bound, taken conservatively in fp32 (the
 *   source says why), exceeds every lane's current best: the result equals the exhaustive one bit for bit.  flags: 0, or for
 *   benchmarks NB_CLOSEST_EXHAUSTIVE (no tile is skipped) | NB_CLOSEST_COUNT_TILES (two uint64 at byte 32 of the scratch
 *   receive the tiles skipped and the tiles met, summed over the waves).  scratch dev, 16-byte aligned:
 *   nb_mesh_closest_scratch_size(V, Nf) bytes (0 for refused sizes).
 *   1 <= P, V, Nf and 3 P, 3 V, 3 Nf < 2^31 - 256, else NB_EINVAL.
 * nb_mesh_rig_bind — one thread per mesh vertex.  model: the BODY; params dev [NB_SMPL_PARAMS]: the bind frame's row; ws dev
 *   [NB_SMPL_WS_FLOATS]: the row the same nb_smpl_pose call left (A_j - [I|0], rot(Rh)); faces dev [Nf,3]: the body's; points
 *   dev [P,3]: the mesh vertices, with face, bary of nb_mesh_closest against the posed body.  Outputs, the rig's arrays in
 *   nb_smpl_model's layout: weights dev [24,P], shapedirs dev [10,3P], v_template dev [P,3]; status dev [4] int32 = {unbound
 *   vertices, degenerate vertices, 0, 0}.
 *   w_j = (b0 (*) W[j,v0] (+) b1 (*) W[j,v1]) (+) b2 (*) W[j,v2];  T = [I|0] + sum_j w_j (A_j - [I|0]), j ascending (nb_smpl_pose's
 *   blend);  y_k = sum_i rot[3i+k] (x_i (-) Th_i), the inverse of its rot . s + Th;  v_shaped = M^-1 ((y (-) t)), M = T[:, :3]
 *   inverted by adjugate over determinant, t = T[:, 3] (blend_utils.py:79-81);  the shape directions interpolated like w_j;
 *   v_template = v_shaped (-) sum_l S_l (*) beta_l, l ascending.  Where !(|det M| >= 2^-10) the vertex is bound rigidly to its
 *   largest-weight joint (the lowest j on a tie): one-hot weights, T = A_j, determinant 1 by construction; status[1] counts
 *   them.  A vertex with face = -1 gets one-hot weights on joint 0, T = A_0 and zero shape directions; status[0] counts them.
 *   Pose blend shapes are not transferred: a rig has posedirs = NULL and is driven with new_params = 0; a bind frame posed with
 *   new_params = 1 has its corrective offsets baked into v_template.  Same size limits, else NB_EINVAL. */
#define NB_CLOSEST_EXHAUSTIVE 1
#define NB_CLOSEST_COUNT_TILES 2
int64_t nb_mesh_closest_scratch_size(int32_t n_verts, int32_t n_faces);
int nb_mesh_closest(const float *points, const float *verts, const int32_t *faces, int32_t n_points, int32_t n_verts,
                    int32_t n_faces, int flags, void *scratch, int64_t scratch_bytes, int32_t *face, float *bary, float *dist2,
                    void *stream);
int nb_mesh_rig_bind(const nb_smpl_model *model, const float *params, const float *ws, const int32_t *faces, int32_t n_faces,
                     const float *points, const int32_t *face, const float *bary, int32_t n_points, float *weights,
                     float *shapedirs, float *v_template, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------
 * Hierarchical sampling behind the march — the per-ray work of the second quadrature of
 * lib/networks/renderer/volume_renderer.py:82-104,117 between nb_march (coarse pass, raw and weights), nb_decode_points (the new
 * points) and nb_composite (n_samples + n_importance samples).  One wave per ray, no atomics: the same inputs give the same bits.
 * Sizes of both entries, else NB_EINVAL: n_samples >= 3 (weights[1:-1] must not be empty), 1 <= n_importance <= 128,
 * n_samples + n_importance <= 512, 0 <= n_rays < 2^31 (n_rays == 0: NB_OK at once).
 * nb_importance_sample — replaces sample_pdf (lib/networks/renderer/nerf_net_utils.py:55-90) as volume_renderer.py:86-90 calls it,
 *   the new points (if_clight_renderer.py:25: o + d * z, :68: d / |d|) and z_std (volume_renderer.py:117).
 *   ray_o, ray_d, near, far, t_vals, t_rand: the march's (nb_march); the coarse depths z are recomputed exactly as the march forms
 *   them, the jitter of t_rand included.  weights dev [n_rays, n_samples]: the coarse pass's.
 *   bins b_j = 0.5 * (z_{j+1} + z_j), j = 0..K with K = n_samples - 2; w_i = weights[i + 1] + 1e-5f, i = 0..K-1; pdf_i = w_i / sum w;
 *   knots c_0 = 0, c_{i+1} = c_i + pdf_i; for each u: inds = #{j: c_j <= u} (searchsorted side='right'), below = max(inds - 1, 0),
 *   above = min(K, inds), denom = c_above - c_below, replaced by 1 where < 1e-5, t = (u - c_below) / denom,
 *   z = b_below + t * (b_above - b_below).  Every operation fp32, rounded once, none contracted; the order of the two sums is written
 *   out at the top of csrc/nb_importance.hip (lane-strided partial sums and a butterfly; a chunked wave scan).
 *   u dev: [n_importance] shared by all rays (u_per_ray == 0: torch.linspace(0, 1, n_importance), the reference's det) or
 *   [n_rays, n_importance] (u_per_ray != 0: torch.rand), any order.
 *   cull HOST pointer or NULL, as nb_march's: with it keep dev [n_rays, n_importance] uint8 receives 1 where the new point
 *   projects inside every silhouette (the march's own test), else 0; keep is NULL iff cull is.  pose dev: nb_scene.pose, read
 *   only when cull->pre_affine (may be NULL otherwise).
 *   outputs dev: z_coarse [n_rays, n_samples] or NULL; z_fine [n_rays, n_importance]; wpts [n_rays, n_importance, 3] =
 *   fl32(o + fl32(d * z)); viewdir [n_rays, n_importance, 3] = d / |d| formed in float64 and rounded once;
 *   z_std [n_rays]: population standard deviation of the ray's z_fine, formed in float64 and rounded once.
 * nb_importance_merge — replaces torch.sort(torch.cat([z_vals, z_samples], -1), -1) (volume_renderer.py:93) for depths that carry
 *   their decoded raw: entry e of the concatenation (coarse, then fine) lands at slot #{j: z_j < z_e} + #{j < e: z_j == z_e}, a stable
 *   sort that needs no sorted input (finite depths).  raw of a fine sample with keep == 0 becomes 0
 *   (if_clight_renderer_mmsk.py:54-59); keep dev or NULL.  z_coarse [n_rays, n_samples], raw_coarse [n_rays, n_samples, 4],
 *   z_fine [n_rays, n_importance], raw_fine [n_rays, n_importance, 4] -> z_vals [n_rays, n_samples + n_importance],
 *   raw [n_rays, n_samples + n_importance, 4]; the three raw arrays 16-byte aligned.
 * ------------------------------------------------------------------------------- */
int nb_importance_sample(const float *ray_o, const float *ray_d, const float *near, const float *far, int64_t n_rays,
                         int32_t n_samples, const float *t_vals, const float *t_rand, const float *weights, int32_t n_importance,
                         const float *u, int u_per_ray, const nb_cull *cull, const float *pose, float *z_coarse, float *z_fine,
                         float *wpts, float *viewdir, uint8_t *keep, float *z_std, void *stream);
int nb_importance_merge(const float *z_coarse, const float *raw_coarse, const float *z_fine, const float *raw_fine,
                        const uint8_t *keep, int64_t n_rays, int32_t n_samples, int32_t n_importance, float *z_vals, float *raw,
                        void *stream);

/* ---------------------------------------------------------------------------------
 * Ray bounds from the posed body: the rays of a rendered camera cut to the body's own depth range instead of its box's.  get_rays
 * (lib/utils/if_nerf/if_nerf_data_utils.py:8-21) forms ray_d = K^-1 (x, y, 1) rotated to the world without normalising it, so when K's
 * last row is (0, 0, 1) the point o + t ray_d has camera depth exactly t, the unit of get_near_far's near and far; the ray of pixel
 * (x, y) passes through the integer point (x, y), the centre of the square nb_smpl_silhouette calls pixel (x, y).  No allocation, no
 * synchronisation, everything on `stream`; every output is a function of the inputs alone (the same bits every call).
 * nb_body_depth_range — nb_smpl_silhouette's arguments, projection, snap, triangle rules and conservative coverage (one device
 *   function projects for both); range dev [F,nv,H,W,2] fp32, 8-byte aligned, a dirty buffer is fine.  A triangle's interval is
 *   [min, max] of the fp32 camera depths (R v + T).z of its three vertices, the values the projection computes (no interpolation).
 *   range[...,0] = the smallest lower end over the triangles covering the pixel, range[...,1] = the largest upper end; a pixel no
 *   triangle covers holds (+inf, -inf).  A (frame, view) that nb_smpl_silhouette declares "does not cull" holds (-inf, +inf) at every
 *   pixel: it does not bound; the other views are unaffected.  Depths are >= 0.01, so their bits order like signed integers: signed
 *   atomic min / max on the bits, no finishing pass.  The same limits on F, V, Nf, nv, H, W; scratch dev, 16-byte aligned:
 *   nb_body_depth_range_scratch_size(F, V, Nf, nv) bytes (0 for refused dimensions).  Five stream operations, as nb_smpl_silhouette.
 * nb_depth_range_widen — range_in dev [n,H,W,2] -> range_out (another buffer), both 8-byte aligned, no NaN in range_in.  First every
 *   pixel takes the minimum of the lower ends and the maximum of the upper ends over the border x border window centred on it, pixels
 *   outside the image ignored (nb_mask_dilate's window; border odd, 1..255): the clothing margin in pixels.  Then every aligned
 *   tile x tile block (origin pixel (0, 0), edge blocks partial; tile 1, 2, 4, 8 or 16) takes the min / max over its pixels, so that
 *   the samples of a depth step of nb_march's 8 x 8 ray tile stay on one depth plane.  Both steps only widen an interval.  One launch.
 * nb_raygen_body — nb_raygen with range dev [H,W,2] (8-byte aligned) and margin (metres, finite, >= 0): for a pixel with nb_raygen's
 *   fp32 near and far, lo = range0 - margin, hi = range1 + margin (one fp32 operation each), near' = fmaxf(near, lo),
 *   far' = fminf(far, hi); the pixel is kept iff nb_raygen keeps it and near' < far'.  ray_o, ray_d, the compaction in pixel order,
 *   mask_at_box, n_rays and the scratch are nb_raygen's; with (-inf, +inf) everywhere every output bit is nb_raygen's.  NB_EINVAL for
 *   a K whose last row is not exactly (0, 0, 1).
 * ------------------------------------------------------------------------------- */
int64_t nb_body_depth_range_scratch_size(int32_t n_frames, int32_t n_verts, int32_t n_faces, int32_t n_views);
int nb_body_depth_range(const float *verts, const int32_t *faces, const float *cam, int32_t n_frames, int32_t n_verts,
                        int32_t n_faces, int32_t n_views, int32_t H, int32_t W, void *scratch, int64_t scratch_bytes, float *range,
                        void *stream);
int nb_depth_range_widen(const float *range_in, int32_t n, int32_t H, int32_t W, int32_t border, int32_t tile, float *range_out,
                         void *stream);
int nb_raygen_body(int32_t H, int32_t W, const double K[9], const double R[9], const double T[3], const float bounds[6],
                   const float *range, float margin, float *ray_o, float *ray_d, float *near, float *far, uint8_t *mask_at_box,
                   int32_t *n_rays, void *scratch, void *stream);

/* ---------------------------------------------------------------------------------
 * The vanilla-NeRF baseline (configs/nerf/nerf_313.yaml: lib/networks/nerf.py and lib/networks/renderer/volume_renderer.py), inference
 * only: the 8 x 256 coordinate MLP with its skip connection and view branch as one kernel, and the depth-only merge its fine pass
 * needs.  The supported network is the one the reference ships: D = 8, W = 256, skips = [4], use_viewdirs, xyz_res 10, view_res 4.
 * No allocation, no synchronisation, everything on `stream`, no atomics: the same inputs give the same bits.
 * nb_nerf_params — HOST struct of DEVICE pointers to one Nerf module's parameters in the reference's shapes (nerf.py:27-43), fp32,
 *   row-major [out, in]: pts_w[0] [256,63], pts_w[1..4,6,7] [256,256], pts_w[5] [256,319] (columns [input_pts 63, h 256], nerf.py:53),
 *   pts_b[i] [256]; views_w [128,283] (columns [feature 256, input_views 27], nerf.py:58), views_b [128]; feature_w [256,256],
 *   feature_b [256]; alpha_w [1,256], alpha_b [1]; rgb_w [3,128], rgb_b [3].
 * nb_nerf_pack_size(precision) — floats of the packed blob (the same for both precisions; 0 for any other).
 * nb_nerf_pack — writes the blob once: the ten matrices in MFMA fragment order with the skip and view layers' columns permuted to
 *   the kernel's row order and K padded with zeros to a multiple of 16, then the biases and the two heads.  packed dev, 16-byte
 *   aligned.  Eleven launches.
 * nb_nerf_decode — raw [n_rays, n_samples, 4] (rgb before the sigmoid, sigma before the relu: nerf.py:65) at the depths z_vals
 *   [n_rays, n_samples] of the rays ray_o, ray_d [n_rays, 3].  Per sample, in this order:
 *     p = fl32(o + fl32(d * z)) per axis; v = d / |d| formed in float64 and rounded once (nb_importance_sample's definitions);
 *     the embeddings [x, sin(2^k x), cos(2^k x)]_k (embedder.py:26-36), k < 10 for p and k < 4 for v: x / (2 pi) in float64,
 *       scaled exactly, its fractional revolution to the hardware sine (<= 4e-7 absolute against torch.sin / cos of the fp32 argument);
 *     h = relu(pts_linears[i](h)), i = 0..7, with h = [embed(p), h] before layer 5; alpha = alpha_linear(h); feature = feature_linear(h);
 *     rgb = rgb_linear(relu(views_linears[0]([feature, embed(v)]))); raw = [rgb, alpha].
 *   NB_PREC_F32: every product an fp32 fma into an fp32 accumulator that starts at the bias (v_mfma_f32_32x32x2_f32 for the ten
 *   matrices); the summation order is written out at the top of csrc/nb_nerf.hip.  NB_PREC_F16X3 (nb_nerf_* only): the ten matrices
 *   on v_mfma_f32_32x32x16_f16 with fp32 accumulation, weights and activations split into an fp16 head and an fp16 remainder, three
 *   products (head.head + head.remainder + remainder.head); biases and the two heads of the network stay fp32.  fp16's range: an
 *   activation above 65504 becomes inf.  A blob serves the precision it was packed for.  Any other precision is NB_EINVAL.
 *   One workgroup carries 64 samples through all layers in LDS; n_rays * n_samples need not be a multiple of 64.
 *   Sizes, else NB_EINVAL: 0 <= n_rays < 2^31 (n_rays == 0: NB_OK at once), 1 <= n_samples <= 512.  NULL pointers, a packed that is
 *   not 16-byte aligned or another pointer that is not 4-byte aligned: NB_EINVAL with a message.  One launch.
 * nb_importance_merge_z — torch.sort(torch.cat([z_vals, z_samples], -1), -1) (volume_renderer.py:93) for depths alone, as the
 *   baseline's fine pass re-evaluates every merged depth: nb_importance_merge's counting rule (one device function ranks for
 *   both) and sizes, without any raw.  z_coarse [n_rays, n_samples], z_fine [n_rays, n_importance] -> z_vals [n_rays, n_samples +
 *   n_importance].
 *
 * Training (opt-in: nothing above changes).  The training forward is NB_PREC_F32 whatever the inference precision is.
 * nb_nerf_decode_tap — nb_nerf_decode(NB_PREC_F32) that also writes the activation tap: the same raw bit for bit.  tap, dev,
 *   16-byte aligned, row-major [n_rays * n_samples, NB_NERF_TAP_COLS = 2528] fp32, per sample the columns
 *     [0, 2048)      h0 .. h7, the outputs of pts_linears[0..7] after the relu, 256 each;
 *     [2048, 2304)   feature_linear's output;
 *     [2304, 2432)   V, the output of views_linears[0] after the relu;
 *     [2432, 2496)   the 63 point-embedding columns in the reference's order, then one zero;
 *     [2496, 2528)   the 27 direction-embedding columns, then five zeros.
 *   Every slice is a 16-byte-aligned strided matrix (row stride 10112 bytes) that nb_gemm_fused takes as it is.  Sizes and
 *   errors as nb_nerf_decode.  One launch.
 * nb_nerf_pack_bwd_size() — floats of the transposed blob (557696).
 * nb_nerf_pack_bwd — writes the blob of the input-gradient chain once per parameter version: views_w[:, :256]^T (K = 128),
 *   feature_w^T, pts_w[7..1]^T (of pts_w[5] its 256 h columns: the 63 input columns of the skip pass no gradient on) in
 *   nb_nerf_pack's [wave][chunk][feature tile][lane][k-step] fragment order, then rgb_w [3,128] and alpha_w [256] as they are.  Biases
 *   are not read and may be NULL.  packed_bwd dev, 16-byte aligned.  Ten launches.
 * nb_nerf_bwd_chain — the gradient of every pre-activation from d_raw [n_pts, 4] (rgb, sigma), the tap (V and h7 .. h0 as relu
 *   masks: the forward's own stored post-activation values, > 0 passes, exactly 0 does not, as torch.relu) and the blob:
 *     dV = (rgb_w^T d_rgb) . [V > 0];  dfeat = views_w[:, :256]^T dV;  dz7 = (feature_w^T dfeat + alpha_w^T d_sigma) . [h7 > 0];
 *     dz_{L-1} = (pts_w[L]^T dz_L) . [h_{L-1} > 0], L = 7 .. 1.
 *   dtap, dev, 16-byte aligned, row-major [n_pts, NB_NERF_DTAP_COLS = 2432] fp32: [256 i, 256 i + 256) dz_i, i = 0 .. 7;
 *   [2048, 2304) dfeat; [2304, 2432) dV.  Only rows < n_pts are written.  Exact fp32 fma chains from 0 in ascending k
 *   (v_mfma_f32_32x32x2_f32; the order is written out at the top of csrc/nb_nerf_bwd.hip), no atomics.  The parameter gradients are
 *   then dW = dz^T x (nb_gemm_fused, trans_a) and db = column sums of dz (nb_colsum) over slices of the two buffers.
 *   Sizes, else NB_EINVAL: 0 <= n_pts < 2^37 (n_pts == 0: NB_OK at once, no pointer is looked at).  NULL or misaligned pointers:
 *   NB_EINVAL with a message.  One launch.
 *
 * The baseline's mesh pass (lib/networks/nerf_mesh.py behind lib/networks/renderer/volume_mesh_renderer.py): a density at points.
 * nb_nerf_density — alpha [n] = alpha_linear(h7) at the points pts [n, 3], the trunk of the MLP alone (nerf_mesh.py:45-54:
 *   pts_linears[0..7] with the skip, then alpha_linear; no feature_linear, no view layer, no colour head, no direction).  packed is
 *   nb_nerf_pack's blob for the same precision (NB_PREC_F32 or NB_PREC_F16X3): there is no other pack format.  The kernels are
 *   nb_nerf_decode's with the view rows, layers 8 and 9 and the colour head left out: the same 64-sample workgroup, the same LDS
 *   image, the same summation order of every layer and of alpha_linear (four 64-column chains, (p0 + p1) + (p2 + p3), then the
 *   bias), so alpha[i] has the bits of nb_nerf_decode's raw[..., 3] at the same fp32 point, in both arithmetics.  The point is read as
 *   given (nb_nerf_decode forms fl32(o + fl32(d z)); a ray of depth 0 gives o).  Raw alpha_linear output: no relu.
 *   Sizes, else NB_EINVAL: 0 <= n < 2^37 (n == 0: NB_OK at once).  NULL pointers, a packed that is not 16-byte aligned, pts or alpha
 *   not 4-byte aligned, another precision: NB_EINVAL with a message.  One launch, no atomics.
 * nb_nerf_embed_grad — the last step of d alpha / d p: from the gradient d_emb by the 63 point-embedding columns and the forward's
 *   own stored columns emb (x, then per frequency f < 10 the three sines and the three cosines, embedder.py:26-36), per axis a
 *     grad[a] = d_emb[a] + sum_f 2^f (d_emb[3 + 6 f + a] emb[3 + 6 f + 3 + a] - d_emb[3 + 6 f + 3 + a] emb[3 + 6 f + a]),
 *   accumulated in float64 in ascending f (every product of two fp32 is exact there) and rounded once.  emb and d_emb are row-major
 *   with strides emb_stride and d_stride in floats (>= 63; the tap's columns NB_NERF_TAP_PTS.. with stride NB_NERF_TAP_COLS serve
 *   as emb), grad dev [n, 3].  One thread per point, no atomics.  0 <= n < 2^39 (n == 0: NB_OK at once); NULL or pointers that are
 *   not 4-byte aligned, a stride below 63: NB_EINVAL.  One launch.
 * ------------------------------------------------------------------------------- */
#define NB_PREC_F16X3 2 /* nb_nerf_pack / nb_nerf_decode only: fp16 head + remainder, three products, fp32 accumulate */
typedef struct nb_nerf_params {
    const float *pts_w[8], *pts_b[8];
    const float *views_w, *views_b, *feature_w, *feature_b, *alpha_w, *alpha_b, *rgb_w, *rgb_b;
} nb_nerf_params;
int64_t nb_nerf_pack_size(int precision);
int nb_nerf_pack(const nb_nerf_params *params, float *packed, int precision, void *stream);
int nb_nerf_decode(const float *packed, const float *ray_o, const float *ray_d, const float *z_vals, int64_t n_rays,
                   int32_t n_samples, float *raw, int precision, void *stream);
#define NB_NERF_TAP_COLS 2528
#define NB_NERF_DTAP_COLS 2432
int nb_nerf_decode_tap(const float *packed, const float *ray_o, const float *ray_d, const float *z_vals, int64_t n_rays,
                       int32_t n_samples, float *raw, float *tap, void *stream);
int64_t nb_nerf_pack_bwd_size(void);
int nb_nerf_pack_bwd(const nb_nerf_params *params, float *packed_bwd, void *stream);
int nb_nerf_bwd_chain(const float *packed_bwd, const float *tap, const float *d_raw, int64_t n_pts, float *dtap, void *stream);
int nb_importance_merge_z(const float *z_coarse, const float *z_fine, int64_t n_rays, int32_t n_samples, int32_t n_importance,
                          float *z_vals, void *stream);
#define NB_NERF_TAP_PTS 2432 /* first column of the point embedding in the tap */
int nb_nerf_density(const float *packed, const float *pts, int64_t n, float *alpha, int precision, void *stream);
int nb_nerf_embed_grad(const float *emb, int64_t emb_stride, const float *d_emb, int64_t d_stride, int64_t n, float *grad,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NB_HIP_H */
