// edge_information.h -- the host arithmetic of gorio_kf_edge_information (include/gorio_kf_edges.h): from an edge's fitness score to the
// two values on the diagonal of its information matrix.  Restates InformationMatrixCalculator::calc_information_matrix,
// src/radar_graph_slam/information_matrix_calculator.cpp:39-49 ("IMC"), and weight() of its header, lines 39-42, of the Go-RIO sources.
// Host code only, nothing of HIP: apd_keyframes.hip includes it, and so does host/test/edge_information_sequence.cpp, which prints it
// for given scores without a device.
#pragma once
#include <cmath>

#include "../../include/gorio_kf_edges.h"

namespace gorio {

// weight(a, max_x, min_y, max_y, x) of the reference, in double
inline double edge_weight(double a, double max_x, double min_y, double max_y, double x) {
  const double y = (1.0 - std::exp(-a * x)) / (1.0 - std::exp(-a * max_x));
  return min_y + (max_y - min_y) * y;
}

// out[0] = 1 / w_x, out[1] = 1 / w_q.  The const branch (IMC:30-35) divides by the standard deviations themselves, as there.
inline void edge_information_from_score(const gorio_inf_params& p, double fitness_score, double out[2]) {
  if (p.use_const_inf_matrix) {
    out[0] = 1.0 / p.const_stddev_x;
    out[1] = 1.0 / p.const_stddev_q;
    return;
  }
  const double min_var_x = std::pow(p.min_stddev_x, 2);
  const double max_var_x = std::pow(p.max_stddev_x, 2);
  const double min_var_q = std::pow(p.min_stddev_q, 2);
  const double max_var_q = std::pow(p.max_stddev_q, 2);
  const float w_x = (float)edge_weight(p.var_gain_a, p.fitness_score_thresh, min_var_x, max_var_x, fitness_score);  // float w_x, IMC:44
  const float w_q = (float)edge_weight(p.var_gain_a, p.fitness_score_thresh, min_var_q, max_var_q, fitness_score);
  out[0] = 1.0 / (double)w_x;  // Identity(6, 6).array() /= w_x: a double divided by the widened float
  out[1] = 1.0 / (double)w_q;
}

}  // namespace gorio
