// tests/golden/slice_rdo_harness.cpp -- TEST INFRASTRUCTURE, used by make_slice_rdo_golden.py
// only (compiled into a temporary directory against the reference's headers, linked with
// oracle/_ref/libtmc3_ref.so).
//
// One call = one reflectance slice through the reference's AttributeEncoder::encode
// (makeAttributeEncoder) with attribute inter prediction, the encoder option
// attrInterIntraSliceRDO on or off.  With `seed_cache` the same encoder object first codes the
// cloud once under the parameters `lp_cached` (option off), so that its cached LoD structure --
// which the inter candidate runs over -- is NOT the one the slice's own parameters give (the
// intra candidate regenerates from those, AttributeEncoder.cpp:526-530, 558-562).
//
// Out: the reconstruction, the payload, abh.enableAttrInterPred after the call, the size of the
// brick header inside the payload, and what the call left in
// AttributeInterPredParams::distEstimate / rateEstimate.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "Attribute.h"
#include "AttributeCommon.h"
#include "PCCPointSet.h"
#include "PayloadBuffer.h"
#include "io_hls.h"

#include "gpcc_attr_mi355.h"

namespace {

using namespace pcc;

void
fill_aps(const gpcc_lod_params& lp, AttributeParameterSet* aps)
{
  *aps = AttributeParameterSet();
  aps->aps_attr_parameter_set_id = 0;
  aps->aps_seq_parameter_set_id = 0;
  aps->attr_encoding = AttributeEncoding(lp.attr_encoding);
  aps->lod_decimation_type = LodDecimationMethod(lp.lod_decimation_type);
  aps->canonical_point_order_flag = false;
  aps->max_points_per_sort_log2_plus1 = 0;
  aps->num_pred_nearest_neighbours_minus1 = lp.num_pred_nearest_neighbours_minus1;
  aps->max_num_direct_predictors = 0;
  aps->direct_avg_predictor_disabled_flag = false;
  aps->adaptive_prediction_threshold = 0;
  aps->intra_lod_search_range = lp.intra_lod_search_range;
  aps->inter_lod_search_range = lp.inter_lod_search_range;
  aps->predictionWithDistributionEnabled = lp.prediction_with_distribution_enabled != 0;
  aps->quant_neigh_weight = {0, 0, 0};
  aps->lodNeighBias = {lp.lod_neigh_bias[0], lp.lod_neigh_bias[1], lp.lod_neigh_bias[2]};
  aps->intra_lod_prediction_skip_layers = lp.intra_lod_prediction_skip_layers;
  aps->inter_component_prediction_enabled_flag = false;
  aps->last_component_prediction_enabled_flag = false;
  aps->pred_weight_blending_enabled_flag = lp.pred_weight_blending_enabled_flag != 0;
  aps->num_detail_levels_minus1 = lp.num_detail_levels_minus1;
  aps->lodSamplingPeriod.assign(lp.lod_sampling_period, lp.lod_sampling_period + lp.num_detail_levels_minus1 + 1);
  aps->dist2 = lp.dist2;
  aps->aps_slice_dist2_deltas_present_flag = true;
  aps->aps_chroma_qp_offset = 0;
  aps->raht_extension = true;
  aps->scalable_lifting_enabled_flag = false;
  aps->max_neigh_range_minus1 = lp.max_neigh_range_minus1;
  aps->spherical_coord_flag = false;
  aps->attr_coord_scale = {1, 1, 1};
  aps->raw_attr_variable_len_flag = false;
  aps->qpShiftStep = 0;
  aps->raht_enable_code_layer = false;
  aps->raht_inter_prediction_depth_minus1 = 0;
  aps->raht_send_inter_filters = false;
  aps->raht_inter_skip_layers = 0;
}

void
fill_abh(const gpcc_lod_params& lp, const int32_t* layer_qp, int num_layers, int search_range, AttributeBrickHeader* abh)
{
  *abh = AttributeBrickHeader();
  abh->attr_sps_attr_idx = 0;
  abh->attr_attr_parameter_set_id = 0;
  abh->attr_geom_slice_id = 0;
  abh->attr_qp_delta_luma = 0;
  abh->attr_qp_delta_chroma = 0;
  abh->attr_region_bits_minus1 = 0;
  abh->attr_dist2_delta = lp.attr_dist2_delta;
  abh->attrInterPredSearchRange = search_range;
  abh->enableAttrInterPred = true;
  abh->disableAttrInterPredForRefFrame2 = false;
  if (num_layers > 1)
    for (int l = 0; l < num_layers; l++) {
      // layer l's QP = the parameter set's + the slice delta (0) + the layer delta
      abh->attr_layer_qp_delta_luma.push_back(layer_qp[l] - layer_qp[0]);
      abh->attr_layer_qp_delta_chroma.push_back(0);
    }
}

void
fill_cloud(const int32_t* xyz, const int32_t* refl, int n, PCCPointSet3* cloud)
{
  cloud->resize(n);
  cloud->addReflectances();
  for (int i = 0; i < n; i++) {
    (*cloud)[i] = point_t{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    cloud->setReflectance(i, attr_t(refl[i]));
  }
}

}  // namespace

// layer_qp [num_layers]: the QP of each layer (layer_qp[0] = init_qp_minus4 + 4).
// Returns the payload length, < 0 on a bad argument.
extern "C" int
slice_rdo_case(
  const gpcc_lod_params* lp_cached, const gpcc_lod_params* lp_slice, int32_t seed_cache, int32_t rdo,
  const int32_t* layer_qp, int32_t num_layers, int32_t bitdepth, int32_t direct_predictors,
  int32_t aps_threshold, const int32_t* xyz, const int32_t* attrs, int32_t n, const int32_t* xyz_ref,
  const int32_t* attrs_ref, int32_t n_ref, int32_t search_range, int32_t frame_distance, int32_t* recon,
  uint8_t* payload_out, int32_t payload_cap, int32_t* abh_inter_after, int32_t* abh_size, double* dist_after,
  int32_t* rate_after)
{
  if (n <= 0 || n_ref <= 0 || num_layers < 1 || (lp_slice->attr_encoding != 1 && lp_slice->attr_encoding != 2))
    return -1;
  SequenceParameterSet sps;
  sps.cabac_bypass_stream_enabled_flag = false;
  sps.entropy_continuation_enabled_flag = false;
  sps.bypass_bin_coding_without_prob_update = false;
  sps.geometry_axis_order = AxisOrder::kXYZ;
  AttributeDescription desc;
  desc.attr_num_dimensions_minus1 = 0;
  desc.attr_instance_id = 0;
  desc.bitdepth = bitdepth;
  desc.attributeLabel = KnownAttributeLabel::kReflectance;
  sps.attributeSets.push_back(desc);

  auto params_of = [&](const gpcc_lod_params& lp, AttributeParameterSet* aps, AttributeBrickHeader* abh) {
    fill_aps(lp, aps);
    aps->init_qp_minus4 = layer_qp[0] - 4;
    aps->aps_slice_qp_deltas_present_flag = num_layers > 1;
    aps->max_num_direct_predictors = direct_predictors;
    aps->adaptive_prediction_threshold = aps_threshold;
    aps->attrInterPredictionEnabled = true;
    aps->attrInterPredSearchRange = search_range;
    fill_abh(lp, layer_qp, num_layers, search_range, abh);
  };
  auto with_frame = [&](AttributeInterPredParams* ip, bool option) {
    ip->enableAttrInterPred = true;
    ip->attrInterIntraSliceRDO = option;
    ip->frameDistance = frame_distance;
    ip->distEstimate = 0.;
    ip->rateEstimate = 0;
    ip->lambda = 0.;
    fill_cloud(xyz_ref, attrs_ref, n_ref, &ip->referencePointCloud);
  };

  auto enc = makeAttributeEncoder();
  if (seed_cache) {
    AttributeParameterSet aps0;
    AttributeBrickHeader abh0;
    params_of(*lp_cached, &aps0, &abh0);
    PCCPointSet3 cloud0;
    fill_cloud(xyz, attrs, n, &cloud0);
    AttributeInterPredParams ip0;
    with_frame(&ip0, false);
    AttributeContexts ctx0;
    ctx0.reset();
    PayloadBuffer payload0(PayloadType::kAttributeBrick);
    enc->encode(sps, desc, aps0, abh0, ctx0, cloud0, &payload0, ip0);
  }

  AttributeParameterSet aps;
  AttributeBrickHeader abh;
  params_of(*lp_slice, &aps, &abh);
  PCCPointSet3 cloud;
  fill_cloud(xyz, attrs, n, &cloud);
  AttributeInterPredParams ip;
  with_frame(&ip, rdo != 0);
  AttributeContexts ctxEnc;
  ctxEnc.reset();
  PayloadBuffer payload(PayloadType::kAttributeBrick);
  enc->encode(sps, desc, aps, abh, ctxEnc, cloud, &payload, ip);

  for (int i = 0; i < n; i++)
    recon[i] = cloud.getReflectance(i);
  *abh_inter_after = abh.enableAttrInterPred ? 1 : 0;
  int hdr = 0;
  parseAbh(sps, aps, payload, &hdr);
  *abh_size = hdr;
  *dist_after = ip.distEstimate;
  *rate_after = ip.rateEstimate;
  const int len = int(payload.size());
  if (payload_out)
    memcpy(payload_out, payload.data(), std::min(len, payload_cap));
  return len;
}
