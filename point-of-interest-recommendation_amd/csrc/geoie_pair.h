// The pair math of GeoIE shared by the training passes (geoie.hip) and the geo-rule scoring (geoie_score.hip): the float32 distance of a
// POI pair and the power law on it.  One definition, so a trained pair and a scored pair are the same bits.
#pragma once
#include "poi_common.h"

namespace poi {

// cal_dis of Load_Data_GeoIE.py:28-42 (FPMC-LR's): float64 in its operation order, cos(lat) from the host (cphi), rounded to float32
// as the reference's fmatrix inputs dist_pos / dist_neg are
__device__ __forceinline__ float gi_dist(double lat1, double lon1, double cp1, double lat2, double lon2, double cp2) {
#pragma clang fp contract(off)
  const double pr = 0.017453292519943295;
  const double a = (lat1 - lat2) * pr;
  const double b = (lon1 - lon2) * pr;
  const double c = (1.0 - cos_small(a)) / 2 + cp1 * cp2 * (1.0 - cos_small(b)) / 2;
  return (float)(12742 * asin(sqrt(c)));
}

// f = a d_eff^b and its a / b derivatives; `bad` for d_eff = 0 with b <= 0 (the reference's inf / NaN)
__device__ __forceinline__ void gi_f(float d32, double dmin, double a, double b, double& f, double& fa, double& fb, bool& bad) {
  double d = (double)d32;
  if (d < dmin) d = dmin;
  if (d == 0.0) {
    f = 0.0; fa = 0.0; fb = 0.0;
    if (!(b > 0.0)) bad = true;
    return;
  }
  const double l = log(d), pw = exp(b * l);
  f = a * pw; fa = pw; fb = f * l;
}

}  // namespace poi
