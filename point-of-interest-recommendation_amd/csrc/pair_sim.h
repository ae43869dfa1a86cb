// The float64 pair similarity of two POIs (include/poi_hip.h: poi_diverse_rerank, poi_similar_nearest, and - with the float32 product
// in the cosine's place - poi_similar_topk): the summation order of a row product, the sin^2 Haversine distance and the mix of the two
// parts.  One routine each for every kernel that must give a pair the same bits as the others (diverse.hip, similar.hip).
#pragma once
#include "poi_common.h"

namespace poi {

// x_a . x_b over D float32 columns (D a multiple of 4): four interleaved float64 fma chains over the float4 columns c = 0, 4, 8 ..
// (chain q takes the columns 4 i + q), closed as (a0 + a1) + (a2 + a3) - one order per dim
__device__ __forceinline__ double dot_rows_f64(const float* xa, const float* xb, int D) {
#pragma clang fp contract(off)
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int c = 0; c < D; c += 4) {
    const float4 u = *reinterpret_cast<const float4*>(xa + c), v = *reinterpret_cast<const float4*>(xb + c);
    a0 = fma((double)u.x, (double)v.x, a0); a1 = fma((double)u.y, (double)v.y, a1);
    a2 = fma((double)u.z, (double)v.z, a2); a3 = fma((double)u.w, (double)v.w, a3);
  }
  return (a0 + a1) + (a2 + a3);
}

// great-circle distance (km): 12742 asin(min(1, sqrt(sin^2(dlat pi/360) + cos(lat) cos(wlat) sin^2(dlon pi/360)))), cos(lat) from the host
__device__ __forceinline__ double sin2_dist_km(double lat, double lon, double cp, double wlat, double wlon, double wcp) {
#pragma clang fp contract(off)
  const double sa = sin((lat - wlat) * 0.008726646259971648), sb = sin((lon - wlon) * 0.008726646259971648);      // pi / 360
  const double q = sa * sa + cp * wcp * (sb * sb);
  return 12742.0 * asin(fmin(1.0, sqrt(q)));
}

// the geographic part with its weight: g exp(-d / scale_km)
__device__ __forceinline__ double geo_part(double g, double d, double scale_km) {
#pragma clang fp contract(off)
  return g * exp(-d / scale_km);
}

// sim = g geo + (1 - g) emb from the weighted geographic part; a part with zero weight is not evaluated (GEO / EMB)
template <bool GEO, bool EMB>
__device__ __forceinline__ double sim_mix(double geo_weighted, double omg, double emb) {
#pragma clang fp contract(off)
  if (!EMB) return geo_weighted;
  return GEO ? geo_weighted + omg * emb : omg * emb;
}

}  // namespace poi
