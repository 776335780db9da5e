// Minimal stand-in for radar_graph_slam/keyframe.hpp (see compat/Eigen/Core for the rationale): SCManager reads only the
// keyframe's database index.
#pragma once
#include <cstddef>
#include <memory>

namespace radar_graph_slam {
struct KeyFrame {
  using Ptr = std::shared_ptr<KeyFrame>;
  std::size_t index = 0;
};
}  // namespace radar_graph_slam
