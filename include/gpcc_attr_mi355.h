/* gpcc_attr_mi355.h -- C ABI of the MI355X attribute-transform library.
 *
 * Drop-in boundary for the attribute-transform hot path of TMC13
 * (reference: MPEGGroup/mpeg-pcc-tmc13 @ release-23.0-rc2).  Every entry
 * point names the reference interface it replaces (file:line relative to
 * the reference tree).  Plain pointers and sizes only; no STL, no torch
 * types.  All entry points return 0 on success and a negative
 * gpcc_status on failure; on failure no output buffer holds a valid
 * result and the caller is expected to run the reference CPU function.
 *
 * Two tiers:
 *   - host tier   (gpcc_raht_forward / gpcc_raht_inverse / gpcc_attr_*):
 *     synchronous, caller-owned HOST buffers, exactly the call shape of the
 *     reference free functions, so a replacement translation unit can
 *     forward to it.
 *   - device tier (gpcc_dev_*): the same operations on buffers already
 *     resident in HBM, batched over slices, asynchronous on a HIP stream.
 *     The host tier is implemented on top of it.
 *
 * Limits: at most GPCC_MAX_POINTS points per call (per batch for the device
 * tier) and coordinates in [0, 2^21); beyond them GPCC_ERR_INVALID_ARG.
 */
#ifndef GPCC_ATTR_MI355_H
#define GPCC_ATTR_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 5 (round 5): gpcc_lift_params / gpcc_pred_params grew by the qp_region_* fields (260 bytes each), GPCC_ERR_RANGE and the
 * inter-frame RAHT entries were added.  A caller compares gpcc_abi_version() with this constant before its first call
 * (the shim TUs do, shim/shim_common.hpp process_context): a library built from another header would read parameter
 * blocks of another size. */
#define GPCC_ABI_VERSION 6
#define GPCC_MAX_POINTS (1 << 29) /* 32-bit device indices, stride <= 3 */

#define GPCC_MAX_QP_LAYERS 32
#define GPCC_MAX_QP_REGIONS 8   /* attr_num_regions a slice header can carry here */
#define GPCC_MAX_AC_QP_LAYERS 32

typedef enum gpcc_status {
  GPCC_OK = 0,
  GPCC_ERR_INVALID_ARG = -1,   /* null pointer, n < 0, c not in {1,2,3}, ... */
  GPCC_ERR_UNSUPPORTED = -2,   /* parameter combination kept on the CPU path */
  GPCC_ERR_NO_DEVICE = -3,     /* no gfx950 device / HIP runtime failure     */
  GPCC_ERR_OUT_OF_MEMORY = -4,
  GPCC_ERR_HIP = -5,           /* a HIP call failed; see gpcc_last_error()   */
  GPCC_ERR_UNSORTED = -6,      /* Morton codes not ascending                 */
  GPCC_ERR_RANGE = -7          /* device tier: values left the range of the fast arithmetic path
                                  (gpcc_ctx_set_fast_arith); nothing was written */
} gpcc_status;

/* Flattened RahtPredictionParams (hls.h:439-466) + QpSet
 * (quantization.h:124-139) + the raht_extension flag
 * (AttributeParameterSet, hls.h:782-876), exactly the values
 * AttributeEncoder.cpp:1273/1341 and AttributeDecoder.cpp:595/658 hand to
 * regionAdaptiveHierarchical{,Inverse}Transform. */
typedef struct gpcc_raht_params {
  int32_t raht_prediction_enabled_flag;
  int32_t integer_haar_enable_flag;
  int32_t raht_prediction_threshold0;
  int32_t raht_prediction_threshold1;
  int32_t raht_subnode_prediction_enabled_flag;
  int32_t raht_prediction_search_range;
  int32_t pred_weight_parent[19]; /* RahtPredictionParams::predWeightParent */
  int32_t pred_weight_child[12];  /* RahtPredictionParams::predWeightChild  */
  int32_t raht_extension;         /* aps.raht_extension                     */

  int32_t num_qp_layers;                      /* QpSet::layers.size() >= 1  */
  int32_t layer_qp[GPCC_MAX_QP_LAYERS][2];    /* QpSet::layers[i] = {luma,
                                                 chroma offset}             */
  int32_t max_qp;                             /* QpSet::maxQp               */
  int32_t fixed_point_qp_offset;              /* QpSet::fixedPointQpOffset  */
  int32_t num_ac_qp_layers;                   /* QpSet::rahtAcCoeffQps.size */
  int32_t ac_qp_offset[GPCC_MAX_AC_QP_LAYERS][7][2];
} gpcc_raht_params;

/* Fill pred_weight_parent / pred_weight_child from the five signalled
 * raht_prediction_weights, as RahtPredictionParams::setPredictionWeights
 * does (hls.h:456-465). */
void gpcc_raht_set_prediction_weights(gpcc_raht_params* p, const int32_t w[5]);

/* ------------------------------------------------------------------ */
/* library / device management                                         */

int gpcc_abi_version(void);
/* Human readable description of the most recent failure on this thread. */
const char* gpcc_last_error(void);
/* Forgets the calling thread's message (a caller that reports "the last error" of a sequence of calls
 * clears it in front of the sequence: the shim TUs do, so that a decline without a message of its own
 * never repeats an earlier slice's). */
void gpcc_clear_last_error(void);
/* Number of usable gfx950 devices (0 if none / no HIP runtime). */
int gpcc_device_count(void);

typedef struct gpcc_ctx gpcc_ctx; /* opaque: device, stream, workspace */

/* Create a context bound to HIP device `device`.  `stream` is a
 * hipStream_t passed as void*: NULL = the library creates its own
 * non-blocking stream; to run on the legacy default stream (the one a null
 * hipStream_t means in a launch) pass GPCC_STREAM_LEGACY, HIP's
 * hipStreamLegacy handle.  Work the caller queues on ANOTHER stream is not
 * ordered against the context's.  Workspace grows on demand and is reused. */
#define GPCC_STREAM_LEGACY ((void*)1)
int gpcc_ctx_create(int device, void* stream, gpcc_ctx** out);
void gpcc_ctx_destroy(gpcc_ctx* ctx);
/* Block until all work queued by this context has completed. */
int gpcc_ctx_synchronize(gpcc_ctx* ctx);
/* Bytes of HBM currently held by the context's workspace. */
size_t gpcc_ctx_workspace_bytes(const gpcc_ctx* ctx);
/* Reserve, ahead of the first transform, everything the RAHT entries allocate on demand for
 * calls of up to `max_points` points in up to `max_slices` slices with `max_c` attribute
 * components at the context's current Morton-bits hint (set that first): the device workspace
 * of the largest flag combination, the pooled blocks and the pinned staging buffers; the
 * device memory is written once and the call returns with the device idle.  A codec that
 * creates a context per sequence and then calls once per (slice, attribute) -- the
 * reference's call pattern, tmc3/AttributeEncoder.cpp:1273, 1341 -- calls this once with its
 * largest slice: no transform allocates afterwards (gpcc_ctx_workspace_bytes stays put), so the
 * first call is not followed by the tens of milliseconds a fresh allocation can cost the calls
 * right behind it.  Not needed for correctness: workspace still grows on
 * demand when a call is larger than what was reserved. */
int gpcc_ctx_reserve(gpcc_ctx* ctx, int64_t max_points, int32_t max_slices, int32_t max_c);
/* Device-tier hint: number of significant Morton-code bits (3 x coordinate
 * bits) of the batches that follow; 0 = unknown (63).  Bounds the number of
 * octree levels that are launched; the host tier derives it itself. */
int gpcc_ctx_set_morton_bits(gpcc_ctx* ctx, int32_t bits);

/* The sub-node prediction kernels (the reference's default flags) compute in doubles where doubles
 * are exact -- every product of the Q15 transform below 2^53: attributes of the bit depth max_qp
 * states (51 + 6 (B - 8), tmc3/quantization.cpp:151) in slices with 2 B + ceil(log2 n) <= 36 -- and
 * in int64 otherwise; the results are the same bits (csrc/raht_arith.hpp).  The kernels check the
 * magnitudes: a call whose values leave the range (attributes wider than max_qp says, a decoder fed
 * arbitrary coefficients) writes nothing; the host tier then repeats it in int64 by itself, the
 * device tier reports GPCC_ERR_RANGE at the next synchronisation.  on = 0: int64 always
 * (also GPCC_F64=0 in the environment).  Default: on. */
int gpcc_ctx_set_fast_arith(gpcc_ctx* ctx, int32_t on);

/* What the context's entries have done since it was created -- lets an
 * integrator (and tests/test_shim_dropin.py) tell the device path from a
 * fallback to the reference's CPU function: the replacement translation
 * units (the files under shim/) call the reference only when an entry returns non-zero,
 * and every such return is counted here. */
typedef struct gpcc_ctx_stats_t {
  int64_t calls_ok;          /* entries that returned GPCC_OK                 */
  int64_t calls_unsupported; /* returned GPCC_ERR_UNSUPPORTED (CPU keeps it)  */
  int64_t calls_failed;      /* returned any other error                      */
  int64_t points_ok;         /* points processed by the successful entries    */
} gpcc_ctx_stats_t;
int gpcc_ctx_stats(const gpcc_ctx* ctx, gpcc_ctx_stats_t* out);

/* The predicting encoder with direct predictors iterates its reconstruction pass and the rate
 * model's trajectory towards their fixed point (see gpcc_pred_forward).  out[0] slices coded that
 * way since the context was created, out[1] passes over all of them, out[2] the most passes one
 * slice took, out[3] slices declined at the pass limit: always 0 -- a slice whose passes do not
 * settle is finished by the ordered walk below, none is declined (bench.py's predicting leg
 * reports these). */
int gpcc_ctx_pred_pass_stats(const gpcc_ctx* ctx, int64_t out[4]);

/* The finish of that encoder: a slice that has not settled after GPCC_PRED_REPAIR_AFTER passes
 * (environment, read when the context is created; default 32, at most 64) is completed by a walk
 * in coding order over the decisions the passes left open (see gpcc_pred_forward).  out[0] slices
 * that entered the walk since the context was created, out[1] predictors walked, out[2] stretches
 * walked (a stretch runs from a wrong decision to the predictor where the rate state agrees
 * again), out[3] the longest stretch.  Summed over the lanes of the device tier as the pass
 * statistics are. */
int gpcc_ctx_pred_repair_stats(const gpcc_ctx* ctx, int64_t out[4]);

/* ------------------------------------------------------------------ */
/* host tier: one slice, host buffers, synchronous                      */

/* Replaces pcc::regionAdaptiveHierarchicalTransform (RAHT.h:47-57,
 * RAHT.cpp:1997-2018) for intra slices.
 *   morton  [n]     ascending Morton codes (mortonAddr, PCCMath.h:606)
 *   qp_off  [n][2]  per-point region QP offsets (QpSet::regionQpOffset),
 *                   NULL = all zero
 *   attrs   [n*c]   in: source attributes, row-major; out: reconstruction
 *                   (unclipped, RAHT.cpp:1969-1975)
 *   coeffs  [c*n]   out: quantised coefficients, planar (coeff[k*n+i],
 *                   RAHT.cpp:992-996), traversal order
 */
int gpcc_raht_forward(
  gpcc_ctx* ctx, const gpcc_raht_params* params, const int64_t* morton,
  const int32_t* qp_off, int32_t* attrs, int32_t* coeffs, int32_t n,
  int32_t c);

/* Replaces pcc::regionAdaptiveHierarchicalInverseTransform (RAHT.h:59-69,
 * RAHT.cpp:2037-2058).  coeffs is read, attrs [n*c] is written. */
int gpcc_raht_inverse(
  gpcc_ctx* ctx, const gpcc_raht_params* params, const int64_t* morton,
  const int32_t* qp_off, int32_t* attrs, const int32_t* coeffs, int32_t n,
  int32_t c);

/* RAHT with attribute inter prediction: replaces pcc::regionAdaptiveHierarchicalTransform /
 * ...InverseTransform (RAHT.h:47-69) called with attrInterPredParams.enableAttrInterPred and a reference
 * frame in paramsForInterRAHT (PCCTMC3Common.h:236-298; RAHT.cpp:849-972 estimate_layer_filter,
 * :1165-1198 the two trees in lock step, :1256-1347 per-layer decision, filter taps and block matching,
 * :1504-1549 the frame's block as prediction, :1810-1829 the decision).
 *   morton_ref [n_ref], attrs_ref [n_ref*c]  the reference frame, Morton order (paramsForInterRAHT.
 *                                            mortonCode / attributes)
 *   layer_modes [32], num_modes   attr_layer_code_mode: written by the encoder, read by the decoder
 *   filter_taps [32], num_taps    FilterTaps (quantised): written by the encoder when
 *                                 enable_filter_estimation, read by the decoder
 *                                 (the decoder accepts NULL for an array whose count is 0)
 * Everything else as gpcc_raht_forward / _inverse (qp_off: region QP offsets per point, NULL = none).  On the
 * device: every parameter
 * set, with sub-node prediction (the dependency kernels, the encoder's two candidates of a level as two
 * launches) and with the integer Haar kernel (the frame gets level arrays of its own) -- except, under the
 * Haar kernel, a frame whose tree height differs from the current one's by a non-multiple of three bits
 * (GPCC_ERR_UNSUPPORTED: the CPU keeps the slice).  The
 * per-layer decision compares two sums of doubles the reference accumulates in coding order with log2 of
 * the HOST's libm inside: the library fills its log2 table from the same libm and adds in the same order
 * (csrc/raht_inter.hpp); a coefficient magnitude beyond the table (2^20) returns GPCC_ERR_UNSUPPORTED. */
typedef struct gpcc_raht_inter_params {
  int32_t raht_inter_prediction_depth_minus1;
  int32_t raht_enable_inter_intra_layer_rdo;
  int32_t enable_filter_estimation;
  int32_t skip_init_layers_for_filtering;
} gpcc_raht_inter_params;

int gpcc_raht_forward_inter(
  gpcc_ctx* ctx, const gpcc_raht_params* params, const gpcc_raht_inter_params* inter,
  const int64_t* morton, const int32_t* qp_off, int32_t* attrs, int32_t* coeffs, int32_t n, int32_t c,
  const int64_t* morton_ref, const int32_t* attrs_ref, int32_t n_ref,
  int32_t* layer_modes, int32_t* num_modes, int32_t* filter_taps, int32_t* num_taps);

int gpcc_raht_inverse_inter(
  gpcc_ctx* ctx, const gpcc_raht_params* params, const gpcc_raht_inter_params* inter,
  const int64_t* morton, const int32_t* qp_off, int32_t* attrs, const int32_t* coeffs, int32_t n, int32_t c,
  const int64_t* morton_ref, const int32_t* attrs_ref, int32_t n_ref,
  const int32_t* layer_modes, int32_t num_modes, const int32_t* filter_taps, int32_t num_taps);

/* Replaces the Morton-code + std::sort(MortonCodeWithIndex) prologue of
 * encode/decode{Colors,Reflectances}TransformRaht
 * (AttributeEncoder.cpp:1225-1229,1316-1321; AttributeDecoder.cpp:538-542,
 * 624-628; ordering MortonCodeWithIndex::operator< PCCTMC3Common.h:184-190:
 * by code, ties by original index).
 *   xyz     [n][3]  point positions (Vec3<int32_t>, non-negative, < 2^21)
 *   morton  [n]     out: sorted codes
 *   order   [n]     out: original index of the i-th sorted point
 */
int gpcc_attr_morton_sort(
  gpcc_ctx* ctx, const int32_t* xyz, int32_t n, int64_t* morton,
  int32_t* order);

/* ------------------------------------------------------------------ */
/* device tier: batched over slices, buffers resident in HBM            */

/* A batch of `num_slices` independent slices laid out back to back.
 * slice s owns points [offsets[s], offsets[s+1]).  offsets is a HOST
 * array of num_slices+1 entries (offsets[0] == 0).  All d_* pointers are
 * device addresses (passed as void* so that no HIP header is needed).
 * For slice s with n_s points and base b = offsets[s]:
 *   d_morton  + b           int64  [n_s]
 *   d_qp_off  + 2*b         int32  [n_s][2]  (d_qp_off may be NULL)
 *   d_attrs   + c*b         int32  [n_s][c]
 *   d_coeffs  + c*b         int32  [c][n_s]   planar per slice
 * The call enqueues work on the context's stream and returns; results
 * are valid after gpcc_ctx_synchronize (or stream ordering). */
int gpcc_dev_raht_forward(
  gpcc_ctx* ctx, const gpcc_raht_params* params, int32_t num_slices,
  const int64_t* offsets, const void* d_morton, const void* d_qp_off,
  void* d_attrs, void* d_coeffs, int32_t c);

int gpcc_dev_raht_inverse(
  gpcc_ctx* ctx, const gpcc_raht_params* params, int32_t num_slices,
  const int64_t* offsets, const void* d_morton, const void* d_qp_off,
  void* d_attrs, const void* d_coeffs, int32_t c);

/* Morton encode + stable sort per slice.  d_xyz int32 [n][3];
 * d_morton int64 [n]; d_order int32 [n] (index local to the slice). */
int gpcc_dev_attr_morton_sort(
  gpcc_ctx* ctx, int32_t num_slices, const int64_t* offsets,
  const void* d_xyz, void* d_morton, void* d_order);

/* ------------------------------------------------------------------ */
/* attribute positions in the pseudo-spherical domain (aps.spherical_coord_flag) */

/* What the reference does to a slice's positions in front of attrEncoder->encode / _attrDecoder->decode
 * (encoder.cpp:1148-1197, decoder.cpp:871-920): convertXyzToRpl (coordinate_conversion.cpp:44-69; findLaser
 * geometry_octree.cpp:856-872, isqrt / iatan2 misc.cpp:139-147, 279-309), the bounding box of the result, and
 * offsetAndScale (coordinate_conversion.cpp:109-118) by the box's minimum and attr_coord_scale.  The result is
 * what gpcc_attr_morton_sort, gpcc_lod_build and the gpcc_*_attr entries take as xyz.
 *
 * Domain: every coordinate less than 2^22 away from laser_origin, every scaled result in [0, 2^21).  A point
 * outside it makes the call (host tier) or the next gpcc_ctx_synchronize (device tier) fail with
 * GPCC_ERR_INVALID_ARG.
 *
 * Not covered, left to the caller's host code: offsetAndScaleShift of the reference frame
 * (coordinate_conversion.cpp:122-144, a few lines over another cloud), the encoder's choice of the scale
 * (normalisedAxesWeights, :73-105) and the second reference of bi-prediction. */
#define GPCC_MAX_LASERS 128 /* cfg/sequences-cat3.yaml lists at most 64 lasersTheta; more -> GPCC_ERR_UNSUPPORTED */

typedef struct gpcc_spherical_params {
  int32_t laser_origin[3];            /* GeometryBrickHeader::geomAngularOrigin(gps) */
  int32_t num_lasers;                 /* gps.angularTheta.size(), >= 1 */
  int32_t laser_theta[GPCC_MAX_LASERS]; /* gps.angularTheta, ascending */
  int32_t attr_coord_scale[3];        /* AttributeParameterSet::attr_coord_scale */
  int32_t min_pos_mode;               /* 0: the bounding box's minimum (intra, encoder.cpp:1186-1188)
                                         1: min_pos as given (zero when aps.attrInterPredictionEnabled; or
                                            the caller's own)
                                         2: min(bounding box's minimum, min_pos) per component
                                            (predgeom + inter, encoder.cpp:1165-1166) */
  int32_t min_pos[3];
  int32_t convert;                    /* 1: xyz -> (r, phi, laser) first; 0: the input is already spherical
                                         (predgeom's _posSph, encoder.cpp:1158-1160): bounding box, offset
                                         and scale only */
} gpcc_spherical_params;

/* Host tier, synchronous.  xyz, pos_out int32 [n][3] (pos_out may be xyz); bbox [6]: min, max of the UNSCALED
 * (r, phi, laser), may be NULL.  On failure neither pos_out nor bbox has been written. */
int gpcc_attr_to_spherical(
  gpcc_ctx* ctx, const gpcc_spherical_params* params, const int32_t* xyz, int32_t n, int32_t* pos_out,
  int32_t* bbox);

/* Device tier: enqueues on the context's stream and returns.  Every slice of the batch gets its own bounding box
 * and minimum.  d_xyz, d_pos_out int32 [n][3], equal or disjoint; d_bbox int32 [num_slices][6], may be NULL. */
int gpcc_dev_attr_to_spherical(
  gpcc_ctx* ctx, const gpcc_spherical_params* params, int32_t num_slices, const int64_t* offsets,
  const void* d_xyz, void* d_pos_out, void* d_bbox);

/* ------------------------------------------------------------------ */
/* the reference frame of an inter-predicted LoD slice                  */

/* What the reference does to the previous frame in front of the lifting and predicting coders of a slice with
 * attribute inter prediction (encoder.cpp:1215-1236, decoder.cpp:926-947): the bounding box of the current
 * slice's attribute-domain positions (computeBoundingBox), and of the WHOLE previous frame in that domain
 * (_refFrameAlt, all slices appended) the points inside the box (Box3::contains, PCCMath.h:469-474, inclusive on
 * all six faces), in order, with their attributes -- an ordered compaction; the order is part of the result.
 * The cropped frame is what gpcc_lod_build_inter and the gpcc_*_attr_inter entries take as xyz_ref / attrs_ref.
 *
 * Domain: every coordinate of the frame and of the slices' boxes in [0, 2^21), as for the Morton sort.  A
 * coordinate outside it makes the call fail with GPCC_ERR_INVALID_ARG (the context's sticky error word; the
 * context works afterwards).
 *
 * Not covered, left to the caller: offsetAndScaleShift (for the LoD coders the reference overwrites the shifted
 * cloud, encoder.cpp:1218) and bi-prediction's merge of two frames (an append). */

/* Device tier.  offsets [num_slices + 1], d_xyz int32 [offsets[num_slices]][3]: the current slices;
 * d_xyz_frame int32 [n_frame][3], d_attrs_frame int32 [n_frame][c], c in 1..3: the previous frame;
 * d_xyz_ref int32 [capacity][3], d_attrs_ref int32 [capacity][c] out: the slices' cropped frames back to back,
 * slice s at [ref_offsets[s], ref_offsets[s + 1]); ref_offsets host int64 [num_slices + 1] out;
 * bbox host int32 [num_slices][6] out (min, max), may be NULL.
 * The call waits ONCE on the context's stream, behind the count and its scan, and fills ref_offsets (and bbox) in
 * every case that got that far; the scatter is enqueued and the call returns.  If ref_offsets[num_slices] >
 * capacity: GPCC_ERR_INVALID_ARG and nothing is written to d_xyz_ref / d_attrs_ref, so that the caller can size
 * the buffers and call again.  A slice may keep nothing (an empty segment: code it with the intra entry).
 * The outputs must not alias the frame (an ordered compaction in place races across tiles): equal pointers give
 * GPCC_ERR_INVALID_ARG.  Argument checks run ahead of the context. */
int gpcc_dev_attr_ref_crop(
  gpcc_ctx* ctx, int32_t num_slices, const int64_t* offsets, const void* d_xyz, int32_t n_frame,
  const void* d_xyz_frame, const void* d_attrs_frame, int32_t c, void* d_xyz_ref, void* d_attrs_ref,
  int64_t capacity, int64_t* ref_offsets, int32_t* bbox);

/* Host tier, one slice, synchronous: upload, the same kernels, download.  xyz [n][3] the current slice;
 * xyz_ref [capacity][3], attrs_ref [capacity][c] out; *n_ref out: the number of points kept (written in every
 * case that got as far as the count, also when it exceeds capacity: GPCC_ERR_INVALID_ARG then, and nothing else
 * is written); bbox [6] out, may be NULL. */
int gpcc_attr_ref_crop(
  gpcc_ctx* ctx, const int32_t* xyz, int32_t n, int32_t n_frame, const int32_t* xyz_frame,
  const int32_t* attrs_frame, int32_t c, int32_t* xyz_ref, int32_t* attrs_ref, int32_t capacity, int32_t* n_ref,
  int32_t* bbox);

/* ------------------------------------------------------------------ */
/* lifting transform (predictors given)                                 */

#define GPCC_MAX_LODS 32

/* What encode/decode{Colors,Reflectances}Lift (AttributeEncoder.cpp:1379-1648,
 * AttributeDecoder.cpp:678-857) read besides the LoD structure: the
 * cumulative LoD sizes (AttributeLods::numPointsInLod, coarse to fine), the
 * QpSet (fixed_point_qp_offset = 24 for lifting, quantization.cpp:155-158),
 * the bit depth for the final clip and the last-component-prediction flag. */
typedef struct gpcc_lift_params {
  int32_t num_lods;
  int32_t num_points_in_lod[GPCC_MAX_LODS];
  int32_t last_component_prediction_enabled_flag;
  int32_t bitdepth;
  int32_t num_qp_layers;
  int32_t layer_qp[GPCC_MAX_QP_LAYERS][2];
  int32_t max_qp;
  int32_t fixed_point_qp_offset;
  /* AttributeParameterSet::scalable_lifting_enabled_flag: the quantisation
   * weight of a predictor is then a function of its level of detail alone
   * (computeQuantizationWeightsScalable, PCCTMC3Common.h:858-891; of a whole
   * slice here, the gpcc_*_partial entries take minGeomNodeSizeLog2 and the
   * slice's point count as arguments) */
  int32_t scalable_lifting_enabled_flag;
  /* QP regions of the slice (AttributeBrickHeader::qpRegions -> QpSet::regions,
   * tmc3/quantization.cpp:100-117), for the entries that build the LoD structure themselves
   * (gpcc_*_encode_attr / _decode_attr, gpcc_dev_*, gpcc_multi_*): every point's offset is derived
   * from its position on the device as QpSet::regionQpOffset does (:195-204: the first region that
   * contains it, bounds inclusive).  gpcc_lift_forward / gpcc_pred_forward and their inverses take the
   * offsets as an array instead and ignore these. */
  int32_t num_qp_regions; /* 0 .. GPCC_MAX_QP_REGIONS */
  int32_t qp_region_min[GPCC_MAX_QP_REGIONS][3];
  int32_t qp_region_max[GPCC_MAX_QP_REGIONS][3];
  int32_t qp_region_offset[GPCC_MAX_QP_REGIONS][2];
} gpcc_lift_params;

/* The predictors of AttributeLods (AttributeCommon.h:89-94) as flat arrays in
 * PREDICTOR order (coding order, coarsest LoD first), after
 * PCCPredictor::computeWeights:
 *   neigh_count [n]     PCCPredictor::neighborCount (0..3)
 *   neigh_index [n][3]  PCCNeighborInfo::predictorIndex (< start of the LoD)
 *   neigh_weight[n][3]  PCCNeighborInfo::weight (8-bit fixed point, sum 256)
 *   indexes     [n]     AttributeLods::indexes: predictor order -> point index
 *   qp_off      [n][2]  region QP offset of each POINT (QpSet::regionQpOffset),
 *                       NULL = none
 * The lifting entries that take the caller's predictors (gpcc_lift_forward,
 * _inverse, _inverse_partial, _forward_inter, _inverse_inter) run a level of
 * detail as one parallel step: every neighbour of a predictor of level l lies
 * in a COARSER level, neigh_index < num_points_in_lod[l - 1], and a predictor
 * of level 0 has none (the reference's assert, PCCTMC3Common.h:805).  Anything
 * else is GPCC_ERR_INVALID_ARG; neighbours in the reference frame (inter_ref)
 * are exempt.  The predicting entries walk the predictors in order and accept
 * any neigh_index below the predictor's own.
 * Forward: replaces the body of encodeColorsLift / encodeReflectancesLift
 * minus the entropy calls.  attrs [n][c] in point order: in source, out the
 * reconstructed (rounded, clipped) attributes, as the reference writes them
 * back with setColor/setReflectance.  coeffs [n][c] out: the quantised
 * values of each predictor in coding order (`values[]`, the input of
 * PCCResidualsEncoder::encode and of the zero-run counter).  lcp_coeffs
 * [GPCC_MAX_LODS] out: AttributeBrickHeader::attrLcpCoeffs (c == 3 and the
 * flag set, otherwise untouched). */
int gpcc_lift_forward(
  gpcc_ctx* ctx, const gpcc_lift_params* params, int32_t n, int32_t c,
  const int32_t* neigh_count, const int32_t* neigh_index,
  const int32_t* neigh_weight, const int32_t* indexes, const int32_t* qp_off,
  int32_t* attrs, int32_t* coeffs, int8_t* lcp_coeffs);

/* Replaces decodeColorsLift / decodeReflectancesLift after the entropy
 * decode: coeffs and lcp_coeffs in, attrs [n][c] (point order) out. */
int gpcc_lift_inverse(
  gpcc_ctx* ctx, const gpcc_lift_params* params, int32_t n, int32_t c,
  const int32_t* neigh_count, const int32_t* neigh_index,
  const int32_t* neigh_weight, const int32_t* indexes, const int32_t* qp_off,
  int32_t* attrs, const int32_t* coeffs, const int8_t* lcp_coeffs);

/* decodeColorsLift / decodeReflectancesLift over the predictors of a PARTIALLY decoded
 * scalable-lifting slice (minGeomNodeSizeLog2 = m > 0, AttributeDecoder.cpp:692-698, 791-797
 * -> computeQuantizationWeightsScalable, PCCTMC3Common.h:858-891): the quantisation weight of
 * a level is geom_num_points / (points up to and including it) with the slice's FULL point
 * count geom_num_points = geom_num_points_minus1 + 1 >= n, and the finest level gets no unit
 * weight (:884).  Everything else is gpcc_lift_inverse over the n predictors given (as built
 * by gpcc_lod_build_partial): coeffs [n][c] are the first n entries of the slice's
 * coefficient sequence, lcp_coeffs are read by the partial structure's own LoD index.
 *   min_geom_node_size_log2 in [0, 20]; > 0 needs params->scalable_lifting_enabled_flag
 *   (GPCC_ERR_INVALID_ARG otherwise).  With 0 and geom_num_points = n: gpcc_lift_inverse. */
int gpcc_lift_inverse_partial(
  gpcc_ctx* ctx, const gpcc_lift_params* params, int32_t n, int32_t c,
  int32_t min_geom_node_size_log2, int32_t geom_num_points,
  const int32_t* neigh_count, const int32_t* neigh_index,
  const int32_t* neigh_weight, const int32_t* indexes, const int32_t* qp_off,
  int32_t* attrs, const int32_t* coeffs, const int8_t* lcp_coeffs);

/* Flattened LoD-generation parameters: the AttributeParameterSet fields
 * buildPredictorsFast reads (hls.h:782-876) plus
 * AttributeBrickHeader::attr_dist2_delta: the parameter block of
 * gpcc_lod_build below. */
typedef struct gpcc_lod_params {
  int32_t attr_encoding;           /* 1 predicting, 2 lifting */
  int32_t lod_decimation_type;     /* LodDecimationMethod */
  int32_t num_detail_levels_minus1;
  int32_t num_pred_nearest_neighbours_minus1;
  int32_t intra_lod_search_range;
  int32_t inter_lod_search_range;
  int32_t prediction_with_distribution_enabled;
  int32_t lod_neigh_bias[3];
  int32_t intra_lod_prediction_skip_layers;
  int32_t dist2;
  int32_t attr_dist2_delta;
  int32_t canonical_point_order_flag;
  int32_t max_points_per_sort_log2_plus1;
  int32_t scalable_lifting_enabled_flag;
  int32_t max_neigh_range_minus1;
  int32_t pred_weight_blending_enabled_flag;
  int32_t lod_sampling_period[GPCC_MAX_LODS];
} gpcc_lod_params;

/* Replaces pcc::AttributeLods::generate (AttributeCommon.h:80-87,
 * AttributeCommon.cpp:44-72 -> buildPredictorsFast PCCTMC3Common.h:2300-2469
 * + PCCPredictor::computeWeights) for one intra slice:
 *   xyz [n][3] point positions (point order, as PCCPointSet3::positions)
 * out, all in PREDICTOR (coding) order, coarsest level of detail first:
 *   neigh_count [n], neigh_index [n][3] (predictor indices), neigh_weight
 *   [n][3] (8-bit weights), indexes [n] (predictor -> point index),
 *   num_points_in_lod [GPCC_MAX_LODS] cumulative, *num_lods.
 * All three decimators (lod_decimation_type 0 distance, 1 periodic, 2
 * centroid) and, for the predicting transform, blendWeights run on the
 * device.  canonical_point_order_flag / max_points_per_sort_log2_plus1
 * (PCCTMC3Common.h:2322-2331: the points taken as they come, or sorted in
 * chunks) are accepted when the points ARE in Morton order -- what the octree
 * geometry coder hands over; then neither changes the result.  Points in any
 * other order with those flags and inter prediction return
 * GPCC_ERR_UNSUPPORTED (the shim keeps them on the reference path).
 * scalable_lifting_enabled_flag (of a whole slice: minGeomNodeSizeLog2 = 0, no
 * points skipped -- gpcc_lod_build_partial is the partial decode) builds the structure of
 * PCCTMC3Common.h:2377-2448: always 21 levels, octree sub-sampling by LoD
 * index, node-corner positions in the search, neighbours beyond
 * max_neigh_range_minus1 dropped, the finer layers searched again while a new
 * layer outweighs them; num_detail_levels_minus1, lod_decimation_type, dist2
 * and the sampling periods are then not read.  neigh_weight entries at and
 * beyond neigh_count are unspecified then (the reference keeps the raw squared
 * distance of a dropped neighbour in its slot; nothing reads it). */
int gpcc_lod_build(
  gpcc_ctx* ctx, const gpcc_lod_params* params, const int32_t* xyz, int32_t n,
  int32_t* neigh_count, int32_t* neigh_index, int32_t* neigh_weight,
  int32_t* indexes, int32_t* num_points_in_lod, int32_t* num_lods);

/* AttributeLods::generate of a PARTIALLY decoded slice (spatial scalability,
 * AttributeCommon.cpp:44-72 with minGeomNodeSizeLog2 = m > 0; buildPredictorsFast,
 * PCCTMC3Common.h:2404-2443): the geometry decoder stopped the octree m levels early
 * (tmc3/decoder.cpp:697-738, geometry_octree_decoder.cpp:2244-2280), xyz [n][3] is the
 * coarser cloud it left (n = P points) and geom_num_points = geom_num_points_minus1 + 1
 * >= n is what the slice header counts.  The level loop runs from LoD m to 20 -- node size,
 * walk direction, corner mask, cell shift and prune distance by the absolute level,
 * num_points_in_lod counted from m -- and the points the decoder never saw count among the
 * finer layers of the "search again" rule (:2424-2425).  Outputs as gpcc_lod_build.
 *   min_geom_node_size_log2 in [0, 20]; > 0 needs scalable_lifting_enabled_flag and
 *   attr_encoding 2 (GPCC_ERR_INVALID_ARG otherwise; the predicting transform returns
 *   GPCC_ERR_UNSUPPORTED: the reference's drivers of it take no m).
 *   With min_geom_node_size_log2 = 0 and geom_num_points = n: exactly gpcc_lod_build. */
int gpcc_lod_build_partial(
  gpcc_ctx* ctx, const gpcc_lod_params* params, const int32_t* xyz, int32_t n,
  int32_t min_geom_node_size_log2, int32_t geom_num_points, int32_t* neigh_count,
  int32_t* neigh_index, int32_t* neigh_weight, int32_t* indexes,
  int32_t* num_points_in_lod, int32_t* num_lods);

/* AttributeLods::generate with attribute INTER prediction
 * (AttributeInterPredParams::enableAttrInterPred; buildPredictorsFast with
 * interRef, PCCTMC3Common.h:2348-2376, 2396-2400; the reference-frame part of
 * computeNearestNeighbors :1270-1292, :1606-1796; updatePredictors :2286-2293;
 * blendWeights :654-656): the neighbour search also takes candidates from the
 * reference frame xyz_ref [n_ref][3] (AttributeInterPredParams::
 * referencePointCloud, point order), search_range =
 * AttributeBrickHeader::attrInterPredSearchRange (it replaces both LoD search
 * ranges of the block), frame_distance = AttributeInterPredParams::
 * frameDistance.  Outputs as gpcc_lod_build, plus inter_ref [n][3]
 * (PCCNeighborInfo::interFrameRef): for a neighbour with the flag set
 * neigh_index is a POINT index of the reference frame (PCCNeighborInfo::
 * pointIndex) and its distance carried the frame distance into the weights.
 * Not combined with scalable lifting / canonical point order
 * (GPCC_ERR_UNSUPPORTED).
 * STATUS (round 3): bit-exact against the oracle on the MI355X
 * (tests/test_zz_gpu_inter_lod.py) and under the CPU wavefront emulator
 * (tests/test_emu_lod.py).  Consumers: gpcc_lift_forward_inter /
 * gpcc_pred_forward_inter (and the inverses) below; the shims call it for
 * slices with attribute inter prediction (seam 2: AttributeLods::generate,
 * seam 3: the operator factories). */
int gpcc_lod_build_inter(
  gpcc_ctx* ctx, const gpcc_lod_params* params, const int32_t* xyz, int32_t n,
  const int32_t* xyz_ref, int32_t n_ref, int32_t search_range,
  int32_t frame_distance, int32_t* neigh_count, int32_t* neigh_index,
  int32_t* neigh_weight, int32_t* indexes, int32_t* num_points_in_lod,
  int32_t* num_lods, int32_t* inter_ref);

/* Reflectance lifting over such a structure (encodeReflectancesLift /
 * decodeReflectancesLift with enableAttrInterPred, AttributeEncoder.cpp:
 * 1543-1648, AttributeDecoder.cpp:780-857; one component -- the reference's
 * colour driver takes no reference frame): predictors and inter_ref as
 * gpcc_lod_build_inter returns them, attrs_ref [n_ref] the reference frame's
 * reflectances in ITS point order.  PCCLiftPredict takes the frame's value
 * for a flagged neighbour; PCCLiftUpdate and the quantisation weights leave
 * it out (PCCTMC3Common.h:735-740, :799-800, :845-846).  Buffers otherwise
 * as gpcc_lift_forward / gpcc_lift_inverse with c = 1.
 * STATUS (round 3): the kernels are the intra ones (the frame's values sit
 * behind the n working values and flagged neighbours point there); that
 * arrangement runs under the CPU emulator against the oracle
 * (tests/test_emu_lod.py) and the entry's first hardware run is
 * tests/test_zz_gpu_inter_lod.py in the round-end tier.
 * A caller that has the slice's positions rather than the structure takes
 * gpcc_lift_encode_attr_inter / gpcc_lift_decode_attr_inter below: build and
 * transform in one call, the structure never leaves the device. */
int gpcc_lift_forward_inter(
  gpcc_ctx* ctx, const gpcc_lift_params* params, int32_t n,
  const int32_t* neigh_count, const int32_t* neigh_index,
  const int32_t* neigh_weight, const int32_t* inter_ref, const int32_t* indexes,
  int32_t* attrs, const int32_t* attrs_ref, int32_t n_ref, int32_t* coeffs);
int gpcc_lift_inverse_inter(
  gpcc_ctx* ctx, const gpcc_lift_params* params, int32_t n,
  const int32_t* neigh_count, const int32_t* neigh_index,
  const int32_t* neigh_weight, const int32_t* inter_ref, const int32_t* indexes,
  int32_t* attrs, const int32_t* attrs_ref, int32_t n_ref,
  const int32_t* coeffs);

/* PCCPredictor::computeWeights (PCCTMC3Common.h:589-633) for n predictors:
 * squared distances in neigh_weight (uint64 [n][3]) -> 8-bit weights
 * (int32 [n][3]); neigh_count is updated in place (far neighbours are
 * dropped). */
int gpcc_lod_compute_weights(
  gpcc_ctx* ctx, int32_t n, int32_t* neigh_count, const uint64_t* dist2,
  int32_t* neigh_weight);

/* Per-kernel timing of the most recent gpcc_dev_raht_* call on this
 * context, measured with HIP events on the context's stream when
 * profiling is enabled (gpcc_ctx_set_profiling(ctx, 1)).  Returns the
 * number of entries written (<= max_entries).  names[i] points to a
 * static string. */
typedef struct gpcc_kernel_time {
  const char* name;
  double total_ms;
  int32_t launches;
} gpcc_kernel_time;
int gpcc_ctx_set_profiling(gpcc_ctx* ctx, int enable);
int gpcc_ctx_kernel_times(
  gpcc_ctx* ctx, gpcc_kernel_time* out, int32_t max_entries);

/* The whole RAHT driver of one slice minus the entropy loop --
 * encodeColorsTransformRaht / encodeReflectancesTransformRaht
 * (tmc3/AttributeEncoder.cpp:1306-1375 / 1214-1302) and
 * decodeColorsRaht / decodeReflectancesRaht (tmc3/AttributeDecoder.cpp:613-674
 * / 527-609): Morton codes of xyz[n][3], sort by (code, index), gather the
 * attributes into that order, transform, clip the reconstruction to
 * [0, 2^bitdepth - 1] and scatter it back by original point index -- one
 * upload, one download, everything in between on the device.
 *   attrs  [n][c] in POINT order: encode in: source, out: clipped
 *          reconstruction; decode out: clipped reconstruction
 *   coeffs planar [c][n] in Morton order, exactly what the entropy loop reads
 * Region QP offsets (QpSet::regionQpOffset) are taken as zero, as in every CTC
 * configuration; use gpcc_attr_morton_sort + gpcc_raht_forward for regions (the LoD-based
 * one-call entries below take the regions in their parameter blocks). */
int gpcc_raht_encode_attr(
  gpcc_ctx* ctx, const gpcc_raht_params* params, const int32_t* xyz,
  int32_t* attrs, int32_t* coeffs, int32_t n, int32_t c, int32_t bitdepth);
int gpcc_raht_decode_attr(
  gpcc_ctx* ctx, const gpcc_raht_params* params, const int32_t* xyz,
  int32_t* attrs, const int32_t* coeffs, int32_t n, int32_t c, int32_t bitdepth);

/* The lifting attribute coder of one slice minus the entropy loop: what
 * AttributeEncoder::encode does for AttributeEncoding::kLiftingTransform --
 * AttributeLods::generate (AttributeEncoder.cpp:575-579) followed by
 * encodeColorsLift / encodeReflectancesLift (:1379-1648) -- resp.
 * AttributeDecoder::decode (AttributeDecoder.cpp:292-296, 678-857), in one
 * call: the LoD structure is built and consumed on the device and never
 * crosses PCIe.
 *   lod     LoD parameters (as for gpcc_lod_build)
 *   lift    in: QP layers, bit depth, last_component_prediction flag;
 *           out: num_lods / num_points_in_lod of the structure that was built
 *   xyz     [n][3] positions, point order
 *   attrs   [n][c] point order; encode in: source, out: clipped
 *           reconstruction; decode out: clipped reconstruction
 *   coeffs  [n][c] coding order (what the entropy loop codes / decoded)
 *   lcp_coeffs [GPCC_MAX_LODS] last-component prediction coefficients
 *   indexes [n] out, may be NULL: predictor -> point index (coding order)
 */
int gpcc_lift_encode_attr(
  gpcc_ctx* ctx, const gpcc_lod_params* lod, gpcc_lift_params* lift,
  const int32_t* xyz, int32_t* attrs, int32_t* coeffs, int8_t* lcp_coeffs,
  int32_t* indexes, int32_t n, int32_t c);
int gpcc_lift_decode_attr(
  gpcc_ctx* ctx, const gpcc_lod_params* lod, gpcc_lift_params* lift,
  const int32_t* xyz, int32_t* attrs, const int32_t* coeffs,
  const int8_t* lcp_coeffs, int32_t* indexes, int32_t n, int32_t c);

/* gpcc_lift_decode_attr of a PARTIALLY decoded scalable-lifting slice
 * (AttributeDecoder::decode with minGeomNodeSizeLog2 = m > 0, AttributeDecoder.cpp:292-296,
 * 678-857): gpcc_lod_build_partial + gpcc_lift_inverse_partial in one call, the structure
 * never leaves the device.  xyz [n][3] is the coarser cloud, coeffs [n][c] the FIRST n
 * entries of the slice's coefficient sequence (the entropy decoder stops there), lcp_coeffs
 * the brick header's, read by the partial structure's own LoD index.  Arguments and checks
 * as gpcc_lod_build_partial; decode only (the encoder always codes whole slices). */
int gpcc_lift_decode_attr_partial(
  gpcc_ctx* ctx, const gpcc_lod_params* lod, gpcc_lift_params* lift,
  const int32_t* xyz, int32_t* attrs, const int32_t* coeffs,
  const int8_t* lcp_coeffs, int32_t* indexes, int32_t n, int32_t c,
  int32_t min_geom_node_size_log2, int32_t geom_num_points);

/* ------------------------------------------------------------------ */
/* predicting transform                                                  */

/* What encode/decode{Colors,Reflectances}Pred (AttributeEncoder.cpp:749-853,
 * 1075-1210, AttributeDecoder.cpp:328-523) read besides the LoD structure:
 * the cumulative LoD sizes, the QpSet (fixed_point_qp_offset = 0 for this
 * transform, quantization.cpp:151-158), the bit depth and the
 * AttributeParameterSet fields of the prediction-mode and inter-component
 * tools (hls.h:782-876). */
typedef struct gpcc_pred_params {
  int32_t num_lods;
  int32_t num_points_in_lod[GPCC_MAX_LODS];
  int32_t bitdepth;
  int32_t num_qp_layers;
  int32_t layer_qp[GPCC_MAX_QP_LAYERS][2];
  int32_t max_qp;
  int32_t max_num_direct_predictors;
  int32_t direct_avg_predictor_disabled_flag;
  int32_t adaptive_prediction_threshold; /* aps.adaptivePredictionThreshold(desc):
                                          * the APS value << max(0, bitdepth - 8) */
  int32_t inter_component_prediction_enabled_flag;
  int32_t quant_neigh_weight[3];
  int32_t max_num_detail_levels;         /* aps.maxNumDetailLevels(): icp_coeffs
                                          * beyond it are zero */
  int32_t scalable_lifting_enabled_flag; /* quantisation weights by level of detail
                                          * (computeQuantizationWeightsScalable,
                                          * PCCTMC3Common.h:858-891) instead
                                          * of quant_neigh_weight */
  /* QP regions of the slice (AttributeBrickHeader::qpRegions -> QpSet::regions,
   * tmc3/quantization.cpp:100-117), for the entries that build the LoD structure themselves
   * (gpcc_*_encode_attr / _decode_attr, gpcc_dev_*, gpcc_multi_*): every point's offset is derived
   * from its position on the device as QpSet::regionQpOffset does (:195-204: the first region that
   * contains it, bounds inclusive).  gpcc_lift_forward / gpcc_pred_forward and their inverses take the
   * offsets as an array instead and ignore these. */
  int32_t num_qp_regions; /* 0 .. GPCC_MAX_QP_REGIONS */
  int32_t qp_region_min[GPCC_MAX_QP_REGIONS][3];
  int32_t qp_region_max[GPCC_MAX_QP_REGIONS][3];
  int32_t qp_region_offset[GPCC_MAX_QP_REGIONS][2];
} gpcc_pred_params;

/* Replaces decodeColorsPred / decodeReflectancesPred after the entropy decode
 * (AttributeDecoder.cpp:328-523), predictors as for gpcc_lift_forward:
 *   values [n][c] in: the decoded `values` of every predictor in coding order
 *          (zero runs expanded; the prediction mode still hidden in their
 *          parities, decodePredModeColor / decodePredModeRefl :288-323,
 *          :404-447)
 *   icp_coeffs [GPCC_MAX_LODS][3] in: AttributeBrickHeader::icpCoeffs (c == 3
 *          and the flag set; otherwise ignored, may be NULL)
 *   attrs  [n][c] out, point order: the reconstruction.
 * A point depends on the reconstruction of its neighbours -- also of its own
 * level of detail unless intra_lod_prediction_skip_layers excludes that: the
 * device walks the dependency DAG (pred_kernels.hpp); the result is the
 * reference's for every configuration, the time grows with the depth of the
 * DAG (a single level of detail on a scan-ordered LiDAR frame is one chain). */
int gpcc_pred_inverse(
  gpcc_ctx* ctx, const gpcc_pred_params* params, int32_t n, int32_t c,
  const int32_t* neigh_count, const int32_t* neigh_index,
  const int32_t* neigh_weight, const int32_t* indexes, const int32_t* qp_off,
  int32_t* attrs, const int32_t* values, const int8_t* icp_coeffs);

/* The reflectance predicting transform over such a structure
 * (encodeReflectancesPred / decodeReflectancesPred with enableAttrInterPred,
 * AttributeEncoder.cpp:749-853, AttributeDecoder.cpp:328-400): every neighbour
 * value the coder reads -- the prediction, the eligibility test of the direct
 * predictors, their evaluation -- is the reference frame's reflectance for a
 * flagged neighbour, and such a neighbour takes no quantisation-weight share.
 * Arguments as gpcc_lift_forward_inter; values as gpcc_pred_forward / _inverse.
 * STATUS (round 3): the DAG pass in its inter build and the spare-entry
 * arrangement run under the CPU emulator against the oracle
 * (tests/test_emu_lod.py); first hardware run: tests/test_zz_gpu_inter_lod.py
 * in the round-end tier.
 * Build and transform in one call: gpcc_pred_encode_attr_inter /
 * gpcc_pred_decode_attr_inter below. */
int gpcc_pred_forward_inter(
  gpcc_ctx* ctx, const gpcc_pred_params* params, int32_t n,
  const int32_t* neigh_count, const int32_t* neigh_index,
  const int32_t* neigh_weight, const int32_t* inter_ref, const int32_t* indexes,
  int32_t* attrs, const int32_t* attrs_ref, int32_t n_ref, int32_t* values);
int gpcc_pred_inverse_inter(
  gpcc_ctx* ctx, const gpcc_pred_params* params, int32_t n,
  const int32_t* neigh_count, const int32_t* neigh_index,
  const int32_t* neigh_weight, const int32_t* inter_ref, const int32_t* indexes,
  int32_t* attrs, const int32_t* attrs_ref, int32_t n_ref,
  const int32_t* values);

/* ------------------------------------------------------------------ */
/* a slice with attribute inter prediction in one call                  */
/* gpcc_lod_build_inter followed by gpcc_lift_forward_inter / gpcc_pred_forward_inter (or the inverses) with the
 * structure left on the device: what AttributeEncoder::encode / AttributeDecoder::decode do for a reflectance
 * slice with enableAttrInterPred minus the entropy loop, for the lifting and the predicting transform.  The same
 * kernels, the same results; the two-call path moves the structure (44 bytes per point) over PCIe twice.
 *   lod         as gpcc_lod_build_inter takes it
 *   lift / pred in: QP layers and tools; out: num_lods / num_points_in_lod, as gpcc_lift_encode_attr
 *   xyz [n][3]; attrs [n] in: the source (encoder), out: the clipped reconstruction, point order
 *   coeffs / values [n] out (encoder) or in (decoder), coding order; indexes [n] out, may be NULL
 *   xyz_ref [n_ref][3], attrs_ref [n_ref], search_range, frame_distance as gpcc_lod_build_inter (the frame
 *               cropped to the slice's box: gpcc_attr_ref_crop)
 * One component by signature.  Checked ahead of the context: a null pointer, n <= 0, n_ref <= 0 or
 * search_range < 0 give GPCC_ERR_INVALID_ARG; scalable lifting, canonical_point_order_flag, a chunked sort or QP
 * regions give GPCC_ERR_UNSUPPORTED.  A declined call leaves the caller's buffers and parameter block untouched. */
int gpcc_lift_encode_attr_inter(
  gpcc_ctx* ctx, const gpcc_lod_params* lod, gpcc_lift_params* lift, const int32_t* xyz, int32_t* attrs,
  int32_t* coeffs, int32_t* indexes, int32_t n, const int32_t* xyz_ref, const int32_t* attrs_ref, int32_t n_ref,
  int32_t search_range, int32_t frame_distance);
int gpcc_lift_decode_attr_inter(
  gpcc_ctx* ctx, const gpcc_lod_params* lod, gpcc_lift_params* lift, const int32_t* xyz, int32_t* attrs,
  const int32_t* coeffs, int32_t* indexes, int32_t n, const int32_t* xyz_ref, const int32_t* attrs_ref,
  int32_t n_ref, int32_t search_range, int32_t frame_distance);
int gpcc_pred_encode_attr_inter(
  gpcc_ctx* ctx, const gpcc_lod_params* lod, gpcc_pred_params* pred, const int32_t* xyz, int32_t* attrs,
  int32_t* values, int32_t* indexes, int32_t n, const int32_t* xyz_ref, const int32_t* attrs_ref, int32_t n_ref,
  int32_t search_range, int32_t frame_distance);
int gpcc_pred_decode_attr_inter(
  gpcc_ctx* ctx, const gpcc_lod_params* lod, gpcc_pred_params* pred, const int32_t* xyz, int32_t* attrs,
  const int32_t* values, int32_t* indexes, int32_t n, const int32_t* xyz_ref, const int32_t* attrs_ref,
  int32_t n_ref, int32_t search_range, int32_t frame_distance);

/* Device tier: a batch in HBM on the context's stream, as gpcc_dev_lift_encode_attr (c = 1, no side
 * coefficients).  lift / pred [num_slices]; d_attrs in place; d_indexes may be NULL.  Slice s takes the frame
 * segment [ref_offsets[s], ref_offsets[s + 1]) of d_xyz_ref int32 [..][3] / d_attrs_ref int32 [..]: exactly what
 * gpcc_dev_attr_ref_crop leaves (ref_offsets host int64 [num_slices + 1]) -- the reference frame of slice t + 1
 * is the reconstruction of frame t, which such a caller has in HBM; nothing of it passes through the host.
 * An empty segment gives GPCC_ERR_INVALID_ARG before any work is enqueued (the reference asserts a non-empty
 * frame: code such a slice with the intra entry).  A frame coordinate outside [0, 2^21) is found on the device:
 * the call returns GPCC_ERR_INVALID_ARG and the context works afterwards.  Other refusals as the host tier's. */
int gpcc_dev_lift_encode_attr_inter(
  gpcc_ctx* ctx, const gpcc_lod_params* lod, gpcc_lift_params* lift, int32_t num_slices, const int64_t* offsets,
  const void* d_xyz, void* d_attrs, void* d_coeffs, void* d_indexes, const int64_t* ref_offsets,
  const void* d_xyz_ref, const void* d_attrs_ref, int32_t search_range, int32_t frame_distance);
int gpcc_dev_lift_decode_attr_inter(
  gpcc_ctx* ctx, const gpcc_lod_params* lod, gpcc_lift_params* lift, int32_t num_slices, const int64_t* offsets,
  const void* d_xyz, void* d_attrs, const void* d_coeffs, void* d_indexes, const int64_t* ref_offsets,
  const void* d_xyz_ref, const void* d_attrs_ref, int32_t search_range, int32_t frame_distance);
int gpcc_dev_pred_encode_attr_inter(
  gpcc_ctx* ctx, const gpcc_lod_params* lod, gpcc_pred_params* pred, int32_t num_slices, const int64_t* offsets,
  const void* d_xyz, void* d_attrs, void* d_values, void* d_indexes, const int64_t* ref_offsets,
  const void* d_xyz_ref, const void* d_attrs_ref, int32_t search_range, int32_t frame_distance);
int gpcc_dev_pred_decode_attr_inter(
  gpcc_ctx* ctx, const gpcc_lod_params* lod, gpcc_pred_params* pred, int32_t num_slices, const int64_t* offsets,
  const void* d_xyz, void* d_attrs, const void* d_values, void* d_indexes, const int64_t* ref_offsets,
  const void* d_xyz_ref, const void* d_attrs_ref, int32_t search_range, int32_t frame_distance);

/* ------------------------------------------------------------------ */
/* slice-level inter / intra decision (attrInterIntraSliceRDO)          */
/* With the encoder option attrInterIntraSliceRDO (TMC3.cpp:1481) a reflectance slice coded with
 * attribute inter prediction by the lifting or the predicting transform is coded TWICE and the
 * cheaper result kept (AttributeEncoder::encode, AttributeEncoder.cpp:501-585;
 * codeAttributeSecondPass(), PCCTMC3Common.h:293-296; only encodeReflectancesLift /
 * encodeReflectancesPred have the second pass):
 *   candidate 0, inter: over the coder object's cached structure, neighbours in the reference
 *     frame allowed (as gpcc_lod_build_inter + gpcc_lift_forward_inter / gpcc_pred_forward_inter);
 *   candidate 1, intra: enableAttrInterPred = false and the structure REGENERATED from this
 *     slice's own aps / abh (:526-530, :558-562), whatever the cache was built with (as
 *     gpcc_lift_encode_attr / gpcc_pred_encode_attr);
 *   distEstimate = sum |reconstruction - source| over the points (:825-827, :1645-1646),
 *   rateEstimate = the length of the arithmetic-coded stream (encoder.stop()),
 *   cost = distEstimate + lambda * rateEstimate, intra wins iff costInter > costIntra.
 *
 * gpcc_lift_encode_attr_rdo / gpcc_pred_encode_attr_rdo run BOTH candidates in one call: positions,
 * attributes and the reference frame are uploaded once, the two structures never leave the
 * device, and one kernel sums both distortions (an int64 sum: exact, and equal to the reference's
 * double, which only ever receives integers below 2^53).
 *   lod_inter   the parameters the cached structure was built with; lod_intra this slice's own
 *   lift / pred in: QP layers and tools (num_lods / num_points_in_lod are not read; not written)
 *   xyz [n][3], attrs [n] the source, NOT written (a declined or failed call leaves the slice
 *               to the CPU path untouched)
 *   xyz_ref [n_ref][3], attrs_ref [n_ref], search_range, frame_distance as gpcc_lod_build_inter
 *   values [2][n] out: each candidate's values in coding order (0 inter, 1 intra)
 *   recon  [2][n] out: each candidate's clipped reconstruction, point order
 *   dist   [2]    out: each candidate's distEstimate
 * One component by signature.  GPCC_ERR_INVALID_ARG (checked ahead of the context): a null
 * pointer, n <= 0, n_ref <= 0, search_range < 0.  GPCC_ERR_UNSUPPORTED as the single-candidate
 * inter entries: scalable lifting, canonical_point_order_flag or a chunked sort in the inter
 * build, QP regions; and a predicting candidate whose mode decisions do not settle
 * (gpcc_pred_forward).  The candidates run one after the other on the context's stream. */
int gpcc_lift_encode_attr_rdo(
  gpcc_ctx* ctx, const gpcc_lod_params* lod_inter, const gpcc_lod_params* lod_intra,
  const gpcc_lift_params* lift, const int32_t* xyz, const int32_t* attrs, int32_t n,
  const int32_t* xyz_ref, const int32_t* attrs_ref, int32_t n_ref, int32_t search_range,
  int32_t frame_distance, int32_t* values, int32_t* recon, int64_t* dist);
int gpcc_pred_encode_attr_rdo(
  gpcc_ctx* ctx, const gpcc_lod_params* lod_inter, const gpcc_lod_params* lod_intra,
  const gpcc_pred_params* pred, const int32_t* xyz, const int32_t* attrs, int32_t n,
  const int32_t* xyz_ref, const int32_t* attrs_ref, int32_t n_ref, int32_t search_range,
  int32_t frame_distance, int32_t* values, int32_t* recon, int64_t* dist);

/* The decision itself, plain host code (no context): AttributeInterPredParams::setLambda /
 * getCost (PCCTMC3Common.h:287-291) verbatim --
 *   lambda = std::pow(0.85 * std::pow(2., (qpMinus4 / 3)), 0.5)   with the INTEGER division,
 *   cost   = distEstimate + lambda * rateEstimate                 in doubles, in this order,
 * and *intra_wins = cost[0] > cost[1] (a tie keeps inter).  bytes_*: the arithmetic-coded length
 * of each candidate (EntropyEncoder::stop()).  cost [2] out: inter, intra. */
int gpcc_slice_rdo_choose(
  int64_t dist_inter, int64_t bytes_inter, int64_t dist_intra, int64_t bytes_intra,
  int32_t init_qp_minus4, int32_t* intra_wins, double* cost);


/* Replaces the body of encodeColorsPred / encodeReflectancesPred minus the
 * entropy calls: attrs in source / out reconstruction, values [n][c] out (the
 * prediction mode in the low bits of the magnitudes, encodePredModeColor /
 * ...Refl), icp_coeffs out (computeInterComponentPredictionCoeffs,
 * AttributeEncoder.cpp:990-1071).  With direct predictors the encoder's mode
 * decision (decidePredModeColor :896-985, decidePredModeRefl :663-745) reads a
 * rate model that every earlier point has updated (:136-222): the device runs
 * the reconstruction pass with the model's states as an input, recomputes the
 * states from the pass's values, and repeats until a pass changes no value --
 * the sequential coder's result (a few passes per slice).  The estimate's log2
 * values come from a table filled by the HOST's libm, so the doubles are the
 * reference's.  Noisy content at low QP leaves a handful of near-tie decisions
 * that chase each other through the rate state from pass to pass: after
 * GPCC_PRED_REPAIR_AFTER passes (default 32) one wavefront walks the predictors
 * in coding order from the first decision that still differs, with the exact
 * rate state, and skips whatever the last pass already has right -- exact and
 * always finite, so no slice is declined for its content
 * (gpcc_ctx_pred_repair_stats).  Every predicting encoder entry below shares
 * this. */
int gpcc_pred_forward(
  gpcc_ctx* ctx, const gpcc_pred_params* params, int32_t n, int32_t c,
  const int32_t* neigh_count, const int32_t* neigh_index,
  const int32_t* neigh_weight, const int32_t* indexes, const int32_t* qp_off,
  int32_t* attrs, int32_t* values, int8_t* icp_coeffs);

/* The predicting attribute coder of one slice minus the entropy loop, as
 * gpcc_lift_encode_attr / gpcc_lift_decode_attr: AttributeLods::generate
 * (with blendWeights when the APS asks for it) and the transform in one call,
 * the predictors never leave the device.  pred: in tools / QP; out num_lods,
 * num_points_in_lod of the structure that was built.  QP regions: the
 * qp_region_* fields of the parameter block (round 4). */
int gpcc_pred_encode_attr(
  gpcc_ctx* ctx, const gpcc_lod_params* lod, gpcc_pred_params* pred,
  const int32_t* xyz, int32_t* attrs, int32_t* values, int8_t* icp_coeffs,
  int32_t* indexes, int32_t n, int32_t c);
int gpcc_pred_decode_attr(
  gpcc_ctx* ctx, const gpcc_lod_params* lod, gpcc_pred_params* pred,
  const int32_t* xyz, int32_t* attrs, const int32_t* values,
  const int8_t* icp_coeffs, int32_t* indexes, int32_t n, int32_t c);

/* gpcc_raht_encode_attr whose result is the symbol stream of the entropy
 * loop (see gpcc_zero_run_pack) instead of the coefficient array: runs [n],
 * values [n][c] (only *num_symbols entries are written and copied), the
 * zero-run formation runs on the device where the coefficients are. */
int gpcc_raht_encode_attr_packed(
  gpcc_ctx* ctx, const gpcc_raht_params* params, const int32_t* xyz,
  int32_t* attrs, int32_t* runs, int32_t* values, int32_t* num_symbols,
  int32_t* trailing_run, int32_t n, int32_t c, int32_t bitdepth);

/* QP regions of a slice (AttributeBrickHeader::qpRegions -> QpSet::regions, quantization.cpp:196-204): the
 * offset of the FIRST box that contains a point is added to its layer QPs.  Field names as in
 * gpcc_lift_params / gpcc_pred_params. */
typedef struct gpcc_qp_regions {
  int32_t num_qp_regions; /* 0 .. GPCC_MAX_QP_REGIONS */
  int32_t qp_region_min[GPCC_MAX_QP_REGIONS][3];
  int32_t qp_region_max[GPCC_MAX_QP_REGIONS][3];
  int32_t qp_region_offset[GPCC_MAX_QP_REGIONS][2];
} gpcc_qp_regions;

/* The RAHT slice drivers with QP regions (round 5): gpcc_raht_encode_attr_packed / gpcc_raht_decode_attr with the
 * per-point offsets the reference's drivers derive with qpSet.regionQpOffset (AttributeEncoder.cpp:1262, 1336;
 * AttributeDecoder.cpp:585, 648) computed on the device from the positions.  regions == NULL or
 * num_qp_regions == 0: exactly the entries without regions. */
int gpcc_raht_encode_attr_packed_regions(
  gpcc_ctx* ctx, const gpcc_raht_params* params, const gpcc_qp_regions* regions, const int32_t* xyz,
  int32_t* attrs, int32_t* runs, int32_t* values, int32_t* num_symbols,
  int32_t* trailing_run, int32_t n, int32_t c, int32_t bitdepth);
int gpcc_raht_decode_attr_regions(
  gpcc_ctx* ctx, const gpcc_raht_params* params, const gpcc_qp_regions* regions, const int32_t* xyz,
  int32_t* attrs, const int32_t* coeffs, int32_t n, int32_t c, int32_t bitdepth);

/* Zero-run formation of a coefficient stream: the part of the reference's
 * entropy loops that is not the arithmetic coder (AttributeEncoder.cpp:
 * 1279-1291 / 1347-1362 RAHT, 1458-1474 / 1617-1633 lifting).  A position
 * whose c values are all zero extends the current run; any other position
 * emits (run, values).  The caller then issues
 *   for k < *num_symbols: encodeRunLength(runs[k]); encode(values[k][0..c));
 *   if (*trailing_run) encodeRunLength(*trailing_run);
 * to the reference's PCCResidualsEncoder -- the bitstream is identical
 * (tests/test_symbols.py) and only the non-zero symbols cross PCIe.
 *   coeffs  planar != 0: [c][n] (RAHT);  planar == 0: [n][c] (lifting)
 *   runs    [n] out (num_symbols used), values [n][c] out
 * Host tier. */
int gpcc_zero_run_pack(
  gpcc_ctx* ctx, const int32_t* coeffs, int32_t n, int32_t c, int32_t planar,
  int32_t* runs, int32_t* values, int32_t* num_symbols, int32_t* trailing_run);

/* estimateDist2 (tmc3/AttributeEncoder.cpp:1684-1720, called from
 * tmc3/encoder.cpp:1203 to derive attr_dist2_delta): for every
 * sampling_period-th point of xyz[n][3] (coded order) the squared distance to
 * the nearest other point within +-search_range positions; the
 * `percentile`-th of those minima picks the smallest shift with
 * 3 << (2*shift) >= dist2.  The distance scan runs on the device, the
 * selection (std::nth_element in the reference) on the host.  Host tier. */
int gpcc_estimate_dist2(
  gpcc_ctx* ctx, const int32_t* xyz, int32_t n, int32_t sampling_period,
  int32_t search_range, float percentile, int32_t* shift_bits);

/* Binarisation of the residual symbols: the part of PCCResidualsEncoder
 * (AttributeEncoder.cpp:57-307 -- encodeRunLength :227-254, encodeSymbol
 * :259-272, encode :278-307, with the exp-Golomb binarisations of
 * entropyutils.h:142-183) that is not the adaptive arithmetic coder.  For the
 * symbol stream of gpcc_zero_run_pack / gpcc_raht_encode_attr_packed (runs,
 * values, trailing run) it returns the binary decisions in coding order, one
 * byte each: (context << 1) | bin with context = 0..4 ctxRunLen[5], 5..18
 * ctxCoeffGtN[2][7], 19..24 ctxCoeffRemPrefix[2][3], 25..30
 * ctxCoeffRemSuffix[2][3] (AttributeCommon.h:54-57), 31 = bypass.  Which
 * context a decision uses depends on the symbol alone, so all symbols are
 * binarised in parallel; the caller's loop is
 *   for (b : bins) ctx(b) == 31 ? enc.encode(bin(b)) : enc.encode(bin(b), model[ctx(b)]);
 * on the reference's own coder: the bitstream is identical (tests/test_bins.py).
 *   c = 3 (colour) or 1;  bins [cap] out;  *num_bins out (also when cap is too
 *   small: the call then fails with GPCC_ERR_INVALID_ARG).  Host tier. */
int gpcc_binarise_symbols(
  gpcc_ctx* ctx, const int32_t* runs, const int32_t* values,
  int32_t num_symbols, int32_t trailing_run, int32_t c, uint8_t* bins,
  int64_t cap, int64_t* num_bins);

/* The entropy front end of the device tier: gpcc_zero_run_pack and gpcc_binarise_symbols for a BATCH of slices whose
 * coefficients are in HBM (what every gpcc_dev_*_encode_attr* entry and gpcc_dev_raht_forward leave), and the way
 * back for the decoders.  Only symbols, decisions and offsets cross PCIe; the number of kernel launches and host
 * waits does not depend on num_slices; workspace comes from the context's arena (gpcc_ctx_reserve covers it).
 *
 * For slice s (n_s points, base b = offsets[s]):
 *   d_coeffs + c*b : planar != 0 -> [c][n_s] (RAHT), planar == 0 -> [n_s][c] (lifting / predicting)
 *   bins of slice s: d_bins[bin_offsets[s] .. bin_offsets[s+1]), the bytes gpcc_binarise_symbols gives
 *   d_runs + b [n_s], d_values + c*b [n_s][c]: symbols of slice s, num_symbols[s] used; both may be NULL
 *   bin_offsets host [num_slices+1]; num_symbols, trailing_run host [num_slices] (may be NULL)
 * The call waits ONCE on the context's stream, between counting and emitting, and fills the host arrays in every
 * case that got that far; the decisions are enqueued behind it and the call returns.
 * bins_capacity < bin_offsets[num_slices]: GPCC_ERR_INVALID_ARG, the host arrays filled, d_bins untouched.
 * d_bins == NULL with bins_capacity == 0 is the sizing call: the same path (GPCC_OK only when there is no decision).
 * Domain: that of the host entries -- c = 1 or 3 (the decisions of a two-component tuple are not defined),
 * |value| <= 2^31 - 1, at most 2^29 points per batch, a non-empty ordered slice table.  Argument checks run ahead
 * of the context.  Zero runs never cross a slice: every slice is a stream of its own. */
int gpcc_dev_residual_bins(
  gpcc_ctx* ctx, int32_t num_slices, const int64_t* offsets, const void* d_coeffs,
  int32_t c, int32_t planar, void* d_bins, int64_t bins_capacity, int64_t* bin_offsets,
  void* d_runs, void* d_values, int32_t* num_symbols, int32_t* trailing_run);

/* runs / values: HOST arrays, slice s owns symbols [sym_offsets[s], sym_offsets[s+1]); the rest of the slice is zero.
 * Writes every position of d_coeffs (layout as above), c in 1..3.  Enqueues and returns, like gpcc_dev_raht_inverse:
 * the symbols have left the caller's arrays when it does.
 * Symbol k of a slice lies at sum_{j<=k} (runs[j] + 1) - 1.  Nothing is stored outside a slice: a negative run, or
 * a symbol at or behind position n_s, is not written and sets the context's sticky error word -- the next
 * gpcc_ctx_synchronize returns GPCC_ERR_INVALID_ARG (the context works afterwards).  A slice with more symbols
 * than points, null or unordered offsets are refused ahead of the context. */
int gpcc_dev_zero_run_unpack(
  gpcc_ctx* ctx, int32_t num_slices, const int64_t* offsets, const int64_t* sym_offsets,
  const int32_t* runs, const int32_t* values, void* d_coeffs, int32_t c, int32_t planar);

/* The RAHT slice coder of the device tier: encode/decode{Colors,Reflectances}TransformRaht
 * (AttributeEncoder.cpp:1214-1302, 1306-1375; AttributeDecoder.cpp:527-609, 613-674) for a BATCH of slices resident
 * in HBM, from point order, in one call: the Morton sort, the gather of the attributes into Morton order, the
 * per-point region QP offsets (QpSet::regionQpOffset), the transform, the clip of the reconstruction to the bit depth
 * and the scatter back by original index.  For slice s (n_s points, base b = offsets[s]):
 *   d_xyz    + 3*b  int32 [n_s][3]  point order, coordinates in [0, 2^21) (not inspected on the host;
 *                                   gpcc_ctx_set_morton_bits is the hint, as for gpcc_dev_attr_morton_sort)
 *   d_attrs  + c*b  int32 [n_s][c]  point order.  Encoder in: the source attributes.  Encoder and decoder out: the
 *                                   reconstruction clipped to [0, 2^bitdepth - 1] -- what gpcc_dev_attr_ref_crop
 *                                   takes as the previous frame
 *   d_coeffs + c*b  int32 [c][n_s]  planar, Morton order: what gpcc_dev_raht_forward leaves and
 *                                   gpcc_dev_residual_bins (planar = 1) / gpcc_dev_zero_run_unpack use
 *   d_order  + b    int32 [n_s]     out, may be NULL: the slice-local original index of the i-th sorted point
 *   regions  host [num_slices], may be NULL: regions[s] are slice s's own boxes; the offset of the first box that
 *            contains a point is added, bounds inclusive.  If no slice names a region (or regions is NULL) the
 *            transform runs without an offset array, exactly as gpcc_dev_raht_forward with d_qp_off == NULL;
 *            otherwise the slices without regions get zeros.  The table is uploaded with the call
 *            (sizeof(gpcc_qp_regions) bytes per slice, in device memory, never a kernel argument).
 * One parameter block serves the batch, as for gpcc_dev_raht_forward.  Per slice the result equals that slice's own
 * gpcc_raht_encode_attr / gpcc_raht_encode_attr_packed_regions / gpcc_raht_decode_attr_regions, whatever stands
 * next to it in the batch.  Neither the launches nor the host waits depend on num_slices, and the call adds no wait
 * to those of gpcc_dev_attr_morton_sort and gpcc_dev_raht_forward; it enqueues and returns, results are valid after
 * gpcc_ctx_synchronize.  A device-side error is the sticky word of the transform.
 * Workspace: what has to outlive the sort and the transform (codes, order, sorted attributes, region offsets, the
 * tables) comes from the context's pool; gpcc_ctx_reserve is NOT extended to it (the first call of a shape
 * allocates, a repeated call allocates nothing).
 * GPCC_ERR_INVALID_ARG, decided on the host ahead of any launch, no byte of the caller's buffers written and the
 * pool whole: a null ctx, params, offsets, d_xyz, d_attrs or d_coeffs; num_slices < 1, offsets[0] != 0, an empty or
 * unordered slice, more than 2^29 points; c outside 1..3 or a parameter block gpcc_dev_raht_forward refuses;
 * bitdepth outside [1, 16]; a num_qp_regions outside [0, GPCC_MAX_QP_REGIONS] in any slice.  All but the null ctx
 * are checked ahead of the context.
 * Not part of these entries: the multi tier, the shim (seam 3 stays on the host-tier entries), bench.py, inter
 * RAHT, per-slice parameter blocks (QP layers per slice), and the host-tier slice driver, which is not re-expressed
 * through these kernels. */
int gpcc_dev_raht_encode_attr(
  gpcc_ctx* ctx, const gpcc_raht_params* params, const gpcc_qp_regions* regions, int32_t num_slices,
  const int64_t* offsets, const void* d_xyz, void* d_attrs, void* d_coeffs, void* d_order, int32_t c,
  int32_t bitdepth);
int gpcc_dev_raht_decode_attr(
  gpcc_ctx* ctx, const gpcc_raht_params* params, const gpcc_qp_regions* regions, int32_t num_slices,
  const int64_t* offsets, const void* d_xyz, void* d_attrs, const void* d_coeffs, void* d_order, int32_t c,
  int32_t bitdepth);

/* ------------------------------------------------------------------ */
/* device tier of the LoD build and the lifting coder                   */
/* The same operations on buffers resident in HBM, num_slices slices back to
 * back (offsets[0] = 0 .. offsets[num_slices] = total points): nothing is
 * allocated per call (workspace from the context's arena) and nothing crosses
 * PCIe except, per level of detail, the size of the retained list the host
 * needs to size the next launches.  Positions are not inspected on the host
 * (coordinates must lie in [0, 2^21)); gpcc_ctx_set_morton_bits bounds the
 * radix passes of the Morton sort.  The slices are processed one after the
 * other on the context's stream; the calls return when the batch is done.
 *
 * gpcc_dev_lod_build: AttributeLods::generate for every slice.
 *   d_xyz [N][3]; out d_neigh_count [N], d_neigh_index [N][3], d_neigh_weight
 *   [N][3], d_indexes [N] -- each slice's in its own predictor order, indices
 *   slice relative; host: num_points_in_lod [num_slices][GPCC_MAX_LODS],
 *   num_lods [num_slices]. */
int gpcc_dev_lod_build(
  gpcc_ctx* ctx, const gpcc_lod_params* params, int32_t num_slices,
  const int64_t* offsets, const void* d_xyz, void* d_neigh_count,
  void* d_neigh_index, void* d_neigh_weight, void* d_indexes,
  int32_t* num_points_in_lod, int32_t* num_lods);

/* gpcc_dev_lift_encode_attr / _decode_attr: gpcc_lift_encode_attr /
 * gpcc_lift_decode_attr for every slice, attributes and coefficients in place
 * in the caller's device buffers.
 *   lift   [num_slices] parameter blocks (in: QP layers etc.; out: the LoD
 *          structure of each slice)
 *   d_attrs [N][c] point order; d_coeffs [N][c] coding order per slice
 *   lcp_coeffs host [num_slices][GPCC_MAX_LODS] (c == 3 and the flag set)
 *   d_indexes [N] out, may be NULL */
int gpcc_dev_lift_encode_attr(
  gpcc_ctx* ctx, const gpcc_lod_params* lod, gpcc_lift_params* lift,
  int32_t num_slices, const int64_t* offsets, const void* d_xyz, void* d_attrs,
  void* d_coeffs, int8_t* lcp_coeffs, void* d_indexes, int32_t c);
int gpcc_dev_lift_decode_attr(
  gpcc_ctx* ctx, const gpcc_lod_params* lod, gpcc_lift_params* lift,
  int32_t num_slices, const int64_t* offsets, const void* d_xyz, void* d_attrs,
  const void* d_coeffs, const int8_t* lcp_coeffs, void* d_indexes, int32_t c);

/* gpcc_dev_lift_forward / _inverse: gpcc_lift_forward / gpcc_lift_inverse for a BATCH of slices over LoD structures
 * the caller already holds in HBM, exactly as gpcc_dev_lod_build wrote them -- so a slice with several attributes
 * on one geometry (colour and reflectance) pays the LoD build once: gpcc_dev_lod_build, then one of these calls per
 * attribute (the reference's cached _lods, AttributeLods::isReusable).  For slice s (n_s points, base
 * b = offsets[s]):
 *   d_neigh_count  + b     int32 [n_s]     predictor order, neighbour indices slice relative
 *   d_neigh_index  + 3*b   int32 [n_s][3]
 *   d_neigh_weight + 3*b   int32 [n_s][3]  after computeWeights
 *   d_indexes      + b     int32 [n_s]     point index of each predictor
 *   d_attrs        + c*b   int32 [n_s][c]  point order.  Forward in: the source.  Forward and inverse out: the
 *                                          reconstruction, rounded and clipped to [0, 2^bitdepth - 1]
 *   d_coeffs       + c*b   int32 [n_s][c]  coding order: the layout of gpcc_dev_lift_encode_attr, which
 *                                          gpcc_dev_residual_bins (planar = 0) reads
 *   d_xyz          + 3*b   int32 [n_s][3]  point order; may be NULL when no slice names a QP region
 *   lift   host [num_slices], input only: num_lods / num_points_in_lod as gpcc_dev_lod_build returned them for the
 *          slice; QP layers, bitdepth, the LCP flag, scalable_lifting_enabled_flag (the quantisation weights of a
 *          whole-slice scalable structure) and the qp_region_* fields are PER SLICE.  Where a slice names regions
 *          the offset of a point is formed on the spot from d_xyz[b + indexes[i]] and the slice's boxes (the first
 *          box that contains the point, bounds inclusive); no [N][2] array is built, slices without regions get zeros.
 *   lcp_coeffs host [num_slices][GPCC_MAX_LODS] (c == 3 and the flag set): forward out, written for the slices
 *          with the flag; inverse in.  May be NULL when no slice needs it.
 * Per slice the results are those of its own gpcc_lift_forward / gpcc_lift_inverse, whatever stands next to it in
 * the batch.  c is 1..3.
 * Launches: a step is one LoD transition of EVERY slice at once (csrc/lift_batch.hpp), so with L the largest
 * num_lods of the batch a forward call is at most 7 + 7 (L - 1) kernel launches and an inverse call at most
 * 5 + 4 (L - 1), whatever num_slices is; the per-slice tables are uploaded once.  The call returns when the batch is
 * done, with exactly one host wait, at its end; the forward call's lcp_coeffs come back with that wait.
 * The structure is not inspected on the host.  A check kernel runs first and states what gpcc_lift_forward checks
 * on the host: counts in 0..3, d_indexes in [0, n_s), every neighbour index in [0, num_points_in_lod[l - 1]) of its
 * predictor's level l.  When it fails no later kernel of the call dereferences anything, the call returns
 * GPCC_ERR_INVALID_ARG and no byte of d_attrs, d_coeffs or lcp_coeffs has been written.
 * Workspace: the working arrays (16 + 16 c bytes per point of the batch), the LCP sums and the tables are blocks of
 * the context's pool; gpcc_ctx_reserve is NOT extended to it (the first call of a shape allocates, a repeated call
 * allocates nothing).
 * GPCC_ERR_INVALID_ARG, decided on the host ahead of any launch, no byte written and the pool whole: a null ctx,
 * lift, offsets, structure array, d_attrs or d_coeffs; num_slices < 1 (or above 2^18), offsets[0] != 0, an empty or
 * unordered slice, more than 2^29 points; c outside 1..3; a lift[s] that gpcc_lift_forward refuses for n_s, or whose
 * num_points_in_lod[0] is negative; a bitdepth outside [1, 16]; a num_qp_regions outside [0, GPCC_MAX_QP_REGIONS];
 * a region in any slice with d_xyz == NULL; the LCP flag with c == 3 and lcp_coeffs == NULL.  All but the null ctx
 * are checked ahead of the context.
 * Not part of these entries: partial decode, inter prediction, the predicting transform, the multi tier, the shim,
 * bench.py.  gpcc_dev_lift_encode_attr is not re-expressed through these kernels. */
int gpcc_dev_lift_forward(
  gpcc_ctx* ctx, const gpcc_lift_params* lift, int32_t num_slices, const int64_t* offsets, const void* d_neigh_count,
  const void* d_neigh_index, const void* d_neigh_weight, const void* d_indexes, const void* d_xyz, void* d_attrs,
  void* d_coeffs, int8_t* lcp_coeffs, int32_t c);
int gpcc_dev_lift_inverse(
  gpcc_ctx* ctx, const gpcc_lift_params* lift, int32_t num_slices, const int64_t* offsets, const void* d_neigh_count,
  const void* d_neigh_index, const void* d_neigh_weight, const void* d_indexes, const void* d_xyz, void* d_attrs,
  const void* d_coeffs, const int8_t* lcp_coeffs, int32_t c);

/* gpcc_dev_lift_decode_attr_partial: gpcc_lift_decode_attr_partial for every slice of a
 * batch resident in HBM.  One min_geom_node_size_log2 for the call (a decoder stops every
 * slice at the same node size); geom_num_points is a HOST array [num_slices], the full
 * point count of each slice (>= its offsets[s + 1] - offsets[s]). */
int gpcc_dev_lift_decode_attr_partial(
  gpcc_ctx* ctx, const gpcc_lod_params* lod, gpcc_lift_params* lift,
  int32_t num_slices, const int64_t* offsets, const void* d_xyz, void* d_attrs,
  const void* d_coeffs, const int8_t* lcp_coeffs, void* d_indexes, int32_t c,
  int32_t min_geom_node_size_log2, const int32_t* geom_num_points);

/* gpcc_dev_pred_encode_attr / _decode_attr: gpcc_pred_encode_attr /
 * gpcc_pred_decode_attr for every slice of a batch resident in HBM (slices
 * concurrent on the context's lanes, as for the lifting coder).
 *   pred   [num_slices] parameter blocks (in: tools, QP; out: the LoD structure)
 *   d_attrs [N][c] point order; d_values [N][c] coding order per slice
 *   icp_coeffs host [num_slices][GPCC_MAX_LODS][3] (c == 3 and the flag set)
 *   d_indexes [N] out, may be NULL.  The encoder with direct predictors as
 *   gpcc_pred_forward: passes, then the ordered walk where they do not settle
 *   (every lane keeps its own statistics, gpcc_ctx_pred_repair_stats adds them up). */
int gpcc_dev_pred_encode_attr(
  gpcc_ctx* ctx, const gpcc_lod_params* lod, gpcc_pred_params* pred,
  int32_t num_slices, const int64_t* offsets, const void* d_xyz, void* d_attrs,
  void* d_values, int8_t* icp_coeffs, void* d_indexes, int32_t c);
int gpcc_dev_pred_decode_attr(
  gpcc_ctx* ctx, const gpcc_lod_params* lod, gpcc_pred_params* pred,
  int32_t num_slices, const int64_t* offsets, const void* d_xyz, void* d_attrs,
  const void* d_values, const int8_t* icp_coeffs, void* d_indexes, int32_t c);

/* ------------------------------------------------------------------ */
/* several GPUs from one host process                                   */
/* Slices are the reference's independent units (tmc3/encoder.cpp:544-571): a
 * single-process C++ host (the reference is one) shards a batch of slices over
 * the GPUs of a node with these entries.  gpcc_multi owns one context per
 * listed device; a call gives every device a contiguous, size-balanced run of
 * the slices, runs the transforms concurrently and gathers reconstructions and
 * coefficients on devices[0] -- RCCL send / receive over xGMI (librccl is
 * loaded on first use) -- the COEFFICIENTS, which feed one arithmetic coder; the
 * reconstruction is downloaded from the device that made it.  The caller's
 * buffers are pinned for the duration of the call (hipHostRegister) so that the
 * uploads of all devices overlap.
 * Listing one physical device several times is allowed (the gather is then a
 * device copy): it exercises the sharding on a one-GPU box.
 *   offsets [num_slices + 1], morton [N] (ascending per slice), attrs [N][c]
 *   (forward: in source, out reconstruction; inverse: out), coeffs planar per
 *   slice as for gpcc_dev_raht_forward.  Region QP offsets are taken as zero. */
typedef struct gpcc_multi gpcc_multi;
int gpcc_multi_create(const int32_t* devices, int32_t num_devices, gpcc_multi** out);
void gpcc_multi_destroy(gpcc_multi* m);
int gpcc_multi_num_devices(const gpcc_multi* m);
int gpcc_multi_uses_rccl(const gpcc_multi* m); /* 1: the gather goes through RCCL */
/* librccl loads, its symbols resolve and a one-rank communicator moves a buffer
 * through ncclSend / ncclRecv on `device` (what a single-GPU box can check of
 * the gather's transport); 0 = fine. */
int gpcc_multi_rccl_selftest(int32_t device);
int gpcc_multi_raht_forward(
  gpcc_multi* m, const gpcc_raht_params* params, int32_t num_slices,
  const int64_t* offsets, const int64_t* morton, int32_t* attrs,
  int32_t* coeffs, int32_t c);
int gpcc_multi_raht_inverse(
  gpcc_multi* m, const gpcc_raht_params* params, int32_t num_slices,
  const int64_t* offsets, const int64_t* morton, int32_t* attrs,
  const int32_t* coeffs, int32_t c);

/* The LoD-based coders on several GPUs: gpcc_lift_encode_attr /
 * gpcc_lift_decode_attr / gpcc_pred_encode_attr / gpcc_pred_decode_attr for every
 * slice of a batch (BASELINE configs[2]: five slices), the slices sharded over
 * the devices as above, each device driven by its own host thread for the
 * duration of the call.  Host buffers: xyz [N][3], attrs [N][c] point order per
 * slice, coeffs / values [N][c] coding order per slice (they feed the host's
 * arithmetic coder, so nothing is gathered between devices), lift / pred
 * [num_slices] parameter blocks (in: QP, tools; out: each slice's LoD structure),
 * lcp_coeffs [num_slices][GPCC_MAX_LODS], icp_coeffs [num_slices][GPCC_MAX_LODS][3],
 * indexes [N] out, may be NULL.  The first failing slice fails the call. */
int gpcc_multi_lift_encode_attr(
  gpcc_multi* m, const gpcc_lod_params* lod, gpcc_lift_params* lift,
  int32_t num_slices, const int64_t* offsets, const int32_t* xyz, int32_t* attrs,
  int32_t* coeffs, int8_t* lcp_coeffs, int32_t* indexes, int32_t c);
int gpcc_multi_lift_decode_attr(
  gpcc_multi* m, const gpcc_lod_params* lod, gpcc_lift_params* lift,
  int32_t num_slices, const int64_t* offsets, const int32_t* xyz, int32_t* attrs,
  const int32_t* coeffs, const int8_t* lcp_coeffs, int32_t* indexes, int32_t c);
int gpcc_multi_pred_encode_attr(
  gpcc_multi* m, const gpcc_lod_params* lod, gpcc_pred_params* pred,
  int32_t num_slices, const int64_t* offsets, const int32_t* xyz, int32_t* attrs,
  int32_t* values, int8_t* icp_coeffs, int32_t* indexes, int32_t c);
int gpcc_multi_pred_decode_attr(
  gpcc_multi* m, const gpcc_lod_params* lod, gpcc_pred_params* pred,
  int32_t num_slices, const int64_t* offsets, const int32_t* xyz, int32_t* attrs,
  const int32_t* values, const int8_t* icp_coeffs, int32_t* indexes, int32_t c);

/* ------------------------------------------------------------------ */
/* attribute transfer ("recolouring") onto a re-quantised geometry       */

/* RecolourParams (tmc3/pointset_processing.h:47-63) + the attribute's bit depth
 * (AttributeDescription::bitdepth, hls.h:286-299).  The reference's defaults
 * (TMC3.cpp:1501-1550): search_range 1, 8 / 1 neighbours, distance-weighted
 * averages, dist offsets 4, every max_*_dist2 1000 (>= 512 means "no limit"),
 * skip_avg_if_identical_fwd 1, _bwd 0. */
typedef struct gpcc_recolour_params {
  double dist_offset_fwd, dist_offset_bwd;
  double max_geometry_dist2_fwd, max_geometry_dist2_bwd;
  double max_attribute_dist2_fwd, max_attribute_dist2_bwd;
  int32_t search_range;
  int32_t num_neighbours_fwd, num_neighbours_bwd; /* 1 .. 8 each */
  int32_t use_dist_weighted_avg_fwd, use_dist_weighted_avg_bwd;
  int32_t skip_avg_if_identical_fwd, skip_avg_if_identical_bwd;
  int32_t bitdepth;
} gpcc_recolour_params;

/* Replaces pcc::recolour (pointset_processing.h:138-144,
 * pointset_processing.cpp:926-957 -> recolourColour :253-594 for c == 3,
 * recolourReflectance :618-916 for c == 1), called by the encoder after geometry
 * quantisation (tmc3/encoder.cpp: the attributes of the source cloud are
 * transferred to the points of the coded geometry).
 *   src_xyz [ns][3], src_attrs [ns][c]   the source cloud (values 0 .. 65535)
 *   tgt_xyz [nt][3]                      the target positions
 *   tgt_attrs [nt][c]                    out
 *   source_to_target_scale, target_to_source_offset[3]:
 *     posInTgt = posInSrc * scale - offset (the reference passes the scale as float)
 * Forward: the K nearest source points of every target point (exact, squared
 * distances in double exactly as nanoflann's L2 adaptor sums them); backward:
 * every source point is appended to the list of its nearest target points; then
 * the blend and the +-search_range refinement of pointset_processing.cpp.
 * PARITY: identical to the reference, equidistant candidates included.  All arithmetic is the
 * reference's (double, same order); where candidates are at EQUAL distance -- on a voxelised cloud
 * at a dyadic scale: at nearly every point -- the reference's result is the order its containers
 * produce, so they are rebuilt on the device: nanoflann's k-d trees (leaf size 10: divideTree /
 * middleSplit_ / planeSplit, dependencies/nanoflann/nanoflann.hpp:872-998) level by level, its search
 * (searchLevel :1308, KNNResultSet::addPoint :175) as a stack walk that visits candidates in
 * nanoflann's order, and the backward lists in source order sorted by libstdc++'s std::sort
 * (introsort, not stable beyond 16 entries).  oracle/recolour_oracle.c restates the same and is
 * pinned to the compiled reference (tests/test_oracle_recolour.py); the device equals both
 * (tests/test_gpu_recolour.py).  Needs ns >= num_neighbours_fwd and
 * nt >= num_neighbours_bwd (else GPCC_ERR_UNSUPPORTED).  A finite
 * max_geometry_dist2_fwd (< 512) is reproduced as the reference behaves (round 5): its result
 * vectors live outside its loop and its test looks at the farthest neighbour FOUND (:292-313), so
 * the first target whose k-th neighbour lies beyond the limit shrinks them to one entry for itself
 * and for every LATER target -- those take the colour of their nearest source point.  A k-d tree
 * deeper than 64 levels is declined (the search's stack).  Host tier. */
int gpcc_recolour(
  gpcc_ctx* ctx, const gpcc_recolour_params* params, const int32_t* src_xyz,
  const int32_t* src_attrs, int32_t ns, const int32_t* tgt_xyz, int32_t nt,
  int32_t c, float source_to_target_scale, const int32_t target_to_source_offset[3],
  int32_t* tgt_attrs);

/* Every attribute of a slice in one call: what the encoder's loop over the attribute sets
 * (tmc3/encoder.cpp:1031-1037, one pcc::recolour per set) computes, for up to GPCC_RC_MAX_ATTRS
 * attributes on the same source and target positions.  attrs[a].tgt receives exactly what
 * gpcc_recolour gives for attribute a alone with params->bitdepth = attrs[a].bitdepth, equidistant
 * candidates included; an attribute's result does not depend on its neighbours in the call.
 * SHARED (run once per call): the uploads of both position arrays, the bounding boxes, both k-d
 * trees, the forward K-NN search of every target, `nearest` / the first limited target under a
 * finite max_geometry_dist2_fwd, the backward search of every source point, the backward lists and
 * their order.  That is exact because none of it reads an attribute: trees, neighbour indices and
 * squared distances depend on positions, scale, offset and the parameters only, and std::sort's
 * comparator (pointset_processing.cpp:416-422 / 770-777) looks at the distance alone, so the
 * permutation it leaves a list in is the same whatever payload rides along.
 * PER ATTRIBUTE: the gather of the neighbours' values, the max_attribute_dist2_* trimming (each
 * attribute starts again from the full list), the averages, the round and the clip to the
 * attribute's own bit depth, the +-search_range refinement; one upload and one download each.
 * params->bitdepth is ignored.  Domain and declines as gpcc_recolour (counts <= 2^27, k 1..8,
 * coordinates in (-2^30, 2^30); ns < num_neighbours_fwd, nt < num_neighbours_bwd or a tree deeper
 * than 64 levels: GPCC_ERR_UNSUPPORTED).  GPCC_ERR_INVALID_ARG ahead of any launch: num_attrs
 * outside 1 .. GPCC_RC_MAX_ATTRS, a c other than 1 or 3, a bit depth outside 1 .. 16, a null
 * pointer, two attributes whose output buffers overlap.  On any failure no output buffer is
 * written, the pooled blocks are back in the pool and the context works afterwards.  Host tier,
 * synchronous: the results come down behind the last kernel, one wait at the end.  The device
 * tier, for a batch of slices per call, is gpcc_dev_recolour_attrs; gpcc_ctx_reserve does not
 * cover the workspace. */
#define GPCC_RC_MAX_ATTRS 4
typedef struct gpcc_recolour_attr {
  const int32_t* src;   /* [ns][c], values 0 .. 65535 */
  int32_t* tgt;         /* [nt][c] out */
  int32_t c;            /* 1 or 3 */
  int32_t bitdepth;     /* 1 .. 16: this attribute's AttributeDescription::bitdepth */
} gpcc_recolour_attr;

int gpcc_recolour_attrs(
  gpcc_ctx* ctx, const gpcc_recolour_params* params, const int32_t* src_xyz, int32_t ns,
  const int32_t* tgt_xyz, int32_t nt, const gpcc_recolour_attr* attrs, int32_t num_attrs,
  float source_to_target_scale, const int32_t target_to_source_offset[3]);

/* Device tier: every attribute of a BATCH of slices in one call, everything resident in HBM -- no
 * position and no attribute crosses PCIe.  Slice s recolours the targets [tgt_offsets[s],
 * tgt_offsets[s + 1]) from the sources [src_offsets[s], src_offsets[s + 1]) of the concatenated
 * arrays: the layout gpcc_src_partition produces as out_offsets and the device-tier coders take as
 * offsets; d_tgt is what gpcc_dev_*_encode_attr take as d_attrs.  For every slice and attribute the
 * output equals what gpcc_recolour_attrs gives for that slice alone, equidistant candidates
 * included; a slice's result does not depend on its neighbours in the batch.
 * The k-d trees of all slices are built as two FORESTS (the sources', the targets'): root r is slice
 * r's tree, all nodes of a level of all trees are split by the same launches, and the host waits on
 * the stream once per level as the host tier does -- neither the launches of any stage nor the waits
 * depend on num_slices.  Per slice, as in the reference: target_to_source_offsets[s], the point
 * counts in the error weights, and under a finite max_geometry_dist2_fwd the first limited target
 * (a limited target shrinks the results of the later targets of ITS slice only).
 * Everything behind the trees is enqueued and the call returns: results are valid after
 * gpcc_ctx_synchronize.  Workspace comes from the context's pool as in the host tier;
 * gpcc_ctx_reserve is NOT extended to it (the first call of a shape allocates).
 * GPCC_ERR_INVALID_ARG, on the host from the offsets and ahead of any launch: everything
 * gpcc_recolour_attrs refuses; offsets that do not ascend from 0 or totals above 2^27; a slice that
 * is empty on one side only (a slice empty on BOTH sides is allowed and skipped); two attributes
 * whose d_tgt ranges overlap, or a d_tgt that is a d_src.  GPCC_ERR_UNSUPPORTED for the call: a
 * non-empty slice with fewer sources than num_neighbours_fwd or fewer targets than
 * num_neighbours_bwd; a tree of any slice deeper than 64 levels.  The slices' bounding boxes are
 * looked at at the build's first wait: a coordinate outside (-2^30, 2^30) is GPCC_ERR_INVALID_ARG.
 * In every failing case no byte of any d_tgt has been written, the pooled blocks are back in the
 * pool and the context works afterwards.
 * Not part of this entry: a device tier of gpcc_quantize_positions / gpcc_src_partition (the caller
 * uploads the partitioned source once, in gpcc_src_partition's layout), the multi tier,
 * gpcc_ctx_reserve, a shim TU (recolouring has no link seam), the per-level host wait (it stays),
 * and the host-tier entries, which are not re-expressed through the forest. */
typedef struct gpcc_dev_recolour_attr {
  const void* d_src;  /* int32 [src_offsets[S]][c], values 0 .. 65535, slices back to back */
  void* d_tgt;        /* int32 [tgt_offsets[S]][c] out: the layout gpcc_dev_*_encode_attr take as d_attrs */
  int32_t c;          /* 1 or 3 */
  int32_t bitdepth;   /* 1 .. 16 */
} gpcc_dev_recolour_attr;

int gpcc_dev_recolour_attrs(
  gpcc_ctx* ctx, const gpcc_recolour_params* params, int32_t num_slices,
  const int64_t* src_offsets, const void* d_src_xyz,   /* host [S+1]; device int32 [.][3] */
  const int64_t* tgt_offsets, const void* d_tgt_xyz,   /* host [S+1]; device int32 [.][3] */
  const gpcc_dev_recolour_attr* attrs, int32_t num_attrs,   /* 1 .. GPCC_RC_MAX_ATTRS */
  float source_to_target_scale,
  const int32_t* target_to_source_offsets);            /* host [S][3]: _originInCodingCoords + _sliceOrigin per slice */

/* ------------------------------------------------------------------ */
/* unique-position quantisation and source partitions                   */

/* What PCCTMC3Encoder3::quantization (encoder.cpp:1554-1577) does to the input cloud in front of the geometry
 * coder.  All arithmetic is float, formed as the reference forms it: int -> float (round to nearest even), one
 * multiplication, roundf (halves away from zero), and
 *   mode 0  quantizePositions (pointset_processing.cpp:170-194): per axis roundf(p * scale) - float(offset) in
 *           float, converted to int32, clipped to [clamp_min, clamp_max]; every point is kept
 *   mode 1  quantizePositionsUniq (:143-159): the same positions; points whose results are equal (after the
 *           clip) merge
 *   mode 2  samplePositionsUniq (:113-134): positions int(roundf(p * scale)) - offset (an integer subtraction, no
 *           clip); points merge where int(roundf(roundf(p * scale) * (sample_scale / scale))) is equal, the
 *           quotient a float division */
typedef struct gpcc_quantize_params {
  int32_t mode;         /* 0 quantizePositions, 1 quantizePositionsUniq, 2 samplePositionsUniq */
  float scale;          /* scaleFactor / quantScale */
  float sample_scale;   /* mode 2 only */
  int32_t offset[3];
  int32_t clamp_min[3], clamp_max[3]; /* modes 0, 1 */
} gpcc_quantize_params;

/* Host tier, synchronous.  src_xyz [n][3]; dst_xyz [n][3] capacity, the first *num_dst points written;
 * idx_to_src [n] capacity, *num_dst entries written: SrcMappedPointSet::idxToSrcIdx; src_dup_next [n], all
 * written: SrcMappedPointSet::srcIdxDupList as reducePointSet (:53-103) returns it.  The source points with equal
 * keys i0 < i1 < ... < ik have src_dup_next[ij] = i(j+1) and src_dup_next[ik] = ik; the destination cloud holds
 * one point per group in the order of the first source indices i0, at the position of src[i0]; idx_to_src[d] = i0.
 * Attributes and laser angles are not touched (the caller gathers laser angles by idx_to_src).
 * Mode 0 writes dst_xyz only, *num_dst = n; idx_to_src and src_dup_next may be NULL.  n == 0 is accepted.
 * Domain: n <= 2^29; scale (and sample_scale, and their float quotient) finite and > 0, clamp_min <= clamp_max,
 * else GPCC_ERR_INVALID_ARG ahead of any launch.  Every float that the reference converts to int32 must lie in
 * [-2^31, 2^31) -- its conversion is undefined outside: a point outside makes the call fail with
 * GPCC_ERR_INVALID_ARG (the context's sticky error word; the context works afterwards) and nothing is written to
 * the caller's buffers.
 * The call waits once on the context's stream behind the count, then exactly *num_dst positions and map entries
 * come down.  Workspace comes from the context's arena and pooled buffers; gpcc_ctx_reserve does NOT cover it
 * (the first call of a size allocates).  There is no device tier: the positions go to the geometry coder on the
 * host, and gpcc_recolour is host tier. */
int gpcc_quantize_positions(
  gpcc_ctx* ctx, const gpcc_quantize_params* params, const int32_t* src_xyz, int32_t n, int32_t* dst_xyz,
  int32_t* idx_to_src, int32_t* src_dup_next, int32_t* num_dst);

/* getPartition(src, map, indexes) (encoder.cpp:1611-1659) for a batch of slices: for every listed destination
 * index, in list order, the source points of its group -- the chain from idx_to_src[index] along src_dup_next
 * until an entry points to itself -- with their positions and attributes.  The output of a slice is what
 * gpcc_recolour takes as its source cloud.
 *   src_xyz [n_src][3], src_attrs [n_src][c] (c 1 or 3)
 *   idx_to_src [n_dst], src_dup_next [n_src]: as gpcc_quantize_positions leaves them
 *   indexes [index_offsets[num_slices]]: slice s lists indexes[index_offsets[s] .. index_offsets[s + 1]); a
 *     slice may be empty, an index may repeat
 *   out_xyz [capacity][3], out_attrs [capacity][c]: the slices back to back, slice s at
 *     [out_offsets[s], out_offsets[s + 1]); out_offsets host int64 [num_slices + 1]
 * src_attrs and out_attrs may both be NULL: positions only.  If capacity is too small, or the outputs are NULL
 * (a call that sizes them): GPCC_ERR_INVALID_ARG with out_offsets filled and nothing written, the convention of
 * gpcc_attr_ref_crop.  An index outside [0, n_dst), a map entry outside [0, n_src) or a src_dup_next entry that
 * does not ascend (next[i] > i, or == i at the end of a chain) is refused with GPCC_ERR_INVALID_ARG (validated on
 * the device as the chains are measured; nothing is written).  At most 2^31 - 1 output points per call.
 * One wait behind the count; the number of launches does not depend on num_slices.  A chain is walked by one
 * lane: a group of g points costs g dependent loads.  gpcc_ctx_reserve does not cover the workspace. */
int gpcc_src_partition(
  gpcc_ctx* ctx, const int32_t* src_xyz, const int32_t* src_attrs, int32_t n_src, int32_t c,
  const int32_t* idx_to_src, int32_t n_dst, const int32_t* src_dup_next, const int32_t* indexes,
  const int32_t* index_offsets, int32_t num_slices, int32_t* out_xyz, int32_t* out_attrs, int64_t capacity,
  int64_t* out_offsets);

/* ------------------------------------------------------------------ */
/* debug / test support (exported by every build; nothing an integrator */
/* needs): used by tests/ and tools/ only                               */
/* ------------------------------------------------------------------ */

/* Allocation events of the context since it was created: out[0] arena (re)allocations, out[1]
 * misses of the pooled device buffers, out[2] / out[3] (re)allocations of the pinned staging of
 * the compact level pass / of the level kernels.  A steady loop shows none. */
int gpcc_debug_alloc_events(const gpcc_ctx* ctx, long long out[4]);
/* Pooled device buffers that are taken at this moment, the lanes of the device tier included:
 * out[0] blocks, out[1] their bytes.  Between calls both are 0: a call returns every block it took. */
int gpcc_debug_pool_in_use(const gpcc_ctx* ctx, long long out[2]);
/* 1 when the library was built with -DGPCC_EXPERIMENTS=1 (opt-in kernel variants compiled in). */
int gpcc_debug_has_experiments(void);
/* Guard bands compared so far in this process (0 unless GPCC_GUARD=1 in the environment). */
unsigned long long gpcc_debug_guard_checks(void);
/* The inter-frame encoder's rate sum (csrc/raht_inter.hpp, rate_sum_kernel) on its own:
 * out[e] = terms[e][0] + terms[e][1] + ... for the two estimates e, doubles added in order. */
int gpcc_debug_rate_sum(gpcc_ctx* ctx, const double* terms, int32_t count, double out[2]);
/* The lossy encoder's RDOQ threshold (csrc/raht_levels.hpp) on its own: for case i out_div[i] =
 * rdoq_threshold(dist2[i], lambda[i], rate_coeff[i], limit[i]) and out_recip[i] = rdoq_threshold_recip
 * of the same with 1 / lambda formed as the kernels form it.  lambda >= 1, dist2 >= 0. */
int gpcc_debug_rdoq_threshold(
  gpcc_ctx* ctx, const int64_t* dist2, const int64_t* lambda, const int32_t* rate_coeff,
  const uint32_t* limit, int64_t count, uint32_t* out_div, uint32_t* out_recip);
/* The zero-run resolver (csrc/raht_rdoq.hpp, rdoq_resolve_kernel) on its own.  offsets [S + 1] are
 * the slices' point offsets; slice s has the ascending, slice-relative cut points
 * cuts[cut_off[s] .. cut_off[s + 1]), consecutive cuts bounding one level's coefficients, levels in
 * coding order (fewer than two cuts: no level).  desc [N] are the RDOQ descriptors, coeffs [N][c]
 * (planar per slice) is resolved in place, slice_l_out [S] receives the last reset carried out of
 * each slice's last level (-1: none). */
int gpcc_debug_rdoq_resolve(
  gpcc_ctx* ctx, int32_t num_slices, const int64_t* offsets, const int32_t* cut_off,
  const int32_t* cuts, const uint32_t* desc, int32_t c, int32_t* coeffs, int32_t* slice_l_out);
/* With GPCC_GUARD=1: writes 16 bytes past a pooled block (mode 0) or an arena sub-allocation
 * (mode 1) ON PURPOSE -- the process must stop with the guard-band message; without guard mode
 * it does nothing.  tests/test_gpu_guard.py runs it in a child process. */
int gpcc_debug_guard_selftest(gpcc_ctx* ctx, int mode);

#ifdef __cplusplus
}
#endif
#endif /* GPCC_ATTR_MI355_H */
