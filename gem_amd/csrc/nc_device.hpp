// nc_device.hpp -- library-internal C++ (not ABI): a node-classification handle over a matrix that is already on the device.  Defined in
// nc.hip; edgeclf.hip hands its pair-feature matrix to the logistic solver through it.
#pragma once
#include <cstdint>

#include "../../include/gem_hip.h"

namespace gemhip {

// What gemhip_nc_create makes from a host matrix, from X_dev [n][ld] float32 on the current device, by one device-to-device copy: the handle
// owns its copy and the caller may free X_dev on return.  1 <= d <= ld, d <= 255, 1 <= n < 2^31, as gemhip_nc_create; the values are NOT
// checked -- the caller vouches that every X_dev[i][c < d] is finite.  Every gemhip_nc_* entry point works on the handle as on any other.
int nc_create_from_device(int64_t n, int32_t d, int64_t ld, const float *X_dev, gemhip_nc_t *out);

}  // namespace gemhip
