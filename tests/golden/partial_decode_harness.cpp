// tests/golden/partial_decode_harness.cpp -- TEST INFRASTRUCTURE, used by
// make_partial_decode_golden.py only (compiled into a temporary directory against the
// reference's headers, linked with oracle/_ref/libtmc3_ref.so).
//
// One call = one fixture case of the spatially scalable ("partial") attribute decode:
//   * the FULL cloud of N points goes through the reference's lifting encoder
//     (makeAttributeEncoder, aps.scalable_lifting_enabled_flag);
//   * the partial cloud of P <= N points (what the geometry decoder leaves when it stops
//     m levels early) goes through AttributeLods::generate(aps, abh, N - 1, m, ...) and
//     through makeAttributeDecoder()->decode(..., N - 1, m, payload, ...).
// Out: the reference's partial LoD structure, its decoded attributes, and the
// last-component-prediction coefficients the decoder read from the brick header.
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

void
fill_cloud(const int32_t* xyz, int n, int c, pcc::PCCPointSet3* cloud)
{
  cloud->resize(n);
  for (int i = 0; i < n; i++)
    (*cloud)[i] = pcc::point_t{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  if (c == 3)
    cloud->addColors();
  else
    cloud->addReflectances();
}

pcc::AttributeInterPredParams
intra_params()
{
  pcc::AttributeInterPredParams ip;
  ip.enableAttrInterPred = false;
  ip.attrInterIntraSliceRDO = false;
  ip.frameDistance = 1;
  return ip;
}

}  // namespace

// layer_qp: [num_layers][2] (luma qp, chroma offset) as gpcc_lift_params::layer_qp.
// Returns the payload length, < 0 on a bad argument.
extern "C" int
partial_decode_case(
  const gpcc_lod_params* lp, const int32_t* layer_qp, int32_t num_layers, int32_t bitdepth,
  int32_t lcp_enabled, const int32_t* xyz_full, const int32_t* attrs_full, int32_t N, int32_t c,
  const int32_t* xyz_part, int32_t P, int32_t m, int32_t* neigh_count, int32_t* neigh_index,
  uint64_t* neigh_weight, int32_t* indexes, int32_t* num_points_in_lod, int32_t* num_lods,
  int32_t* dec_attrs, int8_t* lcp_out)
{
  using namespace pcc;
  if (!lp->scalable_lifting_enabled_flag || lp->attr_encoding != 2 || P > N || (c != 1 && c != 3) || num_layers < 1)
    return -1;
  SequenceParameterSet sps;
  sps.cabac_bypass_stream_enabled_flag = false;
  sps.entropy_continuation_enabled_flag = false;
  sps.bypass_bin_coding_without_prob_update = false;
  sps.geometry_axis_order = AxisOrder::kXYZ;
  AttributeDescription desc;
  desc.attr_num_dimensions_minus1 = c - 1;
  desc.attr_instance_id = 0;
  desc.bitdepth = bitdepth;
  desc.attributeLabel = c == 3 ? KnownAttributeLabel::kColour : KnownAttributeLabel::kReflectance;
  sps.attributeSets.push_back(desc);

  AttributeParameterSet aps = AttributeParameterSet();
  aps.aps_attr_parameter_set_id = 0;
  aps.aps_seq_parameter_set_id = 0;
  aps.attr_encoding = AttributeEncoding::kLiftingTransform;
  aps.lod_decimation_type = LodDecimationMethod::kNone;
  aps.canonical_point_order_flag = false;
  aps.max_points_per_sort_log2_plus1 = 0;
  aps.num_pred_nearest_neighbours_minus1 = lp->num_pred_nearest_neighbours_minus1;
  aps.max_num_direct_predictors = 0;
  aps.direct_avg_predictor_disabled_flag = false;
  aps.adaptive_prediction_threshold = 0;
  aps.intra_lod_search_range = lp->intra_lod_search_range;
  aps.inter_lod_search_range = lp->inter_lod_search_range;
  aps.predictionWithDistributionEnabled = lp->prediction_with_distribution_enabled != 0;
  aps.quant_neigh_weight = {0, 0, 0};
  aps.lodNeighBias = {lp->lod_neigh_bias[0], lp->lod_neigh_bias[1], lp->lod_neigh_bias[2]};
  aps.intra_lod_prediction_skip_layers = lp->intra_lod_prediction_skip_layers;
  aps.inter_component_prediction_enabled_flag = false;
  aps.last_component_prediction_enabled_flag = lcp_enabled != 0 && c == 3;
  aps.pred_weight_blending_enabled_flag = false;
  aps.num_detail_levels_minus1 = lp->num_detail_levels_minus1;
  aps.lodSamplingPeriod.assign(
    lp->lod_sampling_period, lp->lod_sampling_period + lp->num_detail_levels_minus1 + 1);
  aps.dist2 = lp->dist2;
  aps.aps_slice_dist2_deltas_present_flag = false;
  aps.init_qp_minus4 = layer_qp[0] - 4;
  aps.aps_chroma_qp_offset = layer_qp[1];
  aps.aps_slice_qp_deltas_present_flag = num_layers > 1;
  aps.raht_extension = true;
  aps.scalable_lifting_enabled_flag = true;
  aps.max_neigh_range_minus1 = lp->max_neigh_range_minus1;
  aps.spherical_coord_flag = false;
  aps.attr_coord_scale = {1, 1, 1};
  aps.raw_attr_variable_len_flag = false;
  aps.attrInterPredictionEnabled = false;
  aps.attrInterPredSearchRange = 0;
  aps.qpShiftStep = 0;
  aps.raht_enable_code_layer = false;
  aps.raht_inter_prediction_depth_minus1 = 0;
  aps.raht_send_inter_filters = false;
  aps.raht_inter_skip_layers = 0;

  AttributeBrickHeader abh = AttributeBrickHeader();
  abh.attr_sps_attr_idx = 0;
  abh.attr_attr_parameter_set_id = 0;
  abh.attr_geom_slice_id = 0;
  abh.attr_qp_delta_luma = 0;
  abh.attr_qp_delta_chroma = 0;
  abh.attr_region_bits_minus1 = 0;
  abh.attr_dist2_delta = 0;
  abh.attrInterPredSearchRange = 0;
  abh.enableAttrInterPred = false;
  abh.disableAttrInterPredForRefFrame2 = false;
  if (num_layers > 1)
    for (int l = 0; l < num_layers; l++) {
      // layer l's QP = the parameter set's + the slice delta (0) + the layer delta
      abh.attr_layer_qp_delta_luma.push_back(layer_qp[2 * l] - layer_qp[0]);
      abh.attr_layer_qp_delta_chroma.push_back(layer_qp[2 * l + 1] - layer_qp[1]);
    }

  // encode the full cloud
  PCCPointSet3 full;
  fill_cloud(xyz_full, N, c, &full);
  for (int i = 0; i < N; i++) {
    if (c == 3)
      full.setColor(
        i, Vec3<attr_t>{attr_t(attrs_full[3 * i]), attr_t(attrs_full[3 * i + 1]), attr_t(attrs_full[3 * i + 2])});
    else
      full.setReflectance(i, attr_t(attrs_full[i]));
  }
  AttributeContexts ctxEnc, ctxDec;
  ctxEnc.reset();
  ctxDec.reset();
  PayloadBuffer payload(PayloadType::kAttributeBrick);
  auto ipEnc = intra_params();
  makeAttributeEncoder()->encode(sps, desc, aps, abh, ctxEnc, full, &payload, ipEnc);

  // the decoder's view: the brick header re-parsed from the payload
  int abhSize = 0;
  AttributeBrickHeader abh2 = parseAbh(sps, aps, payload, &abhSize);
  memset(lcp_out, 0, GPCC_MAX_LODS);
  for (size_t i = 0; i < abh2.attrLcpCoeffs.size() && i < GPCC_MAX_LODS; i++)
    lcp_out[i] = abh2.attrLcpCoeffs[i];

  PCCPointSet3 part;
  fill_cloud(xyz_part, P, c, &part);
  auto ipDec = intra_params();

  AttributeLods lods;
  lods.generate(aps, abh2, N - 1, m, part, ipDec);
  for (int i = 0; i < P; i++) {
    const auto& p = lods.predictors[i];
    neigh_count[i] = p.neighborCount;
    for (int k = 0; k < 3; k++) {
      neigh_index[3 * i + k] = p.neighbors[k].predictorIndex;
      neigh_weight[3 * i + k] = p.neighbors[k].weight;
    }
    indexes[i] = lods.indexes[i];
  }
  *num_lods = int(lods.numPointsInLod.size());
  for (size_t i = 0; i < lods.numPointsInLod.size(); i++)
    num_points_in_lod[i] = lods.numPointsInLod[i];

  makeAttributeDecoder()->decode(
    sps, desc, aps, abh2, N - 1, m, payload.data() + abhSize, payload.size() - abhSize, ctxDec,
    part, ipDec);
  for (int i = 0; i < P; i++)
    for (int d = 0; d < c; d++)
      dec_attrs[c * i + d] = c == 3 ? part.getColor(i)[d] : part.getReflectance(i);
  return int(payload.size());
}
