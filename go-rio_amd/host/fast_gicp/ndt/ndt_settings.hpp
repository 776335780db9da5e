// Drop-in for the reference's fast_gicp/ndt/ndt_settings.hpp: the distance mode of fast_gicp::NDTCuda, in the order of
// gorio_ndt_cuda_distance (include/gorio_apd.h).
#ifndef FAST_GICP_NDT_SETTINGS_HPP
#define FAST_GICP_NDT_SETTINGS_HPP

namespace fast_gicp {

enum class NDTDistanceMode { P2D, D2D };

}  // namespace fast_gicp

#endif
