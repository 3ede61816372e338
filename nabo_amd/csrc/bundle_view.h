// bundle_view.h -- what another translation unit of the library may read of a nabo_bundle (bundle.hip owns the struct): the
// present polylines as they lie on the device, and the numbers nabo_bundle_result de-normalises them with.
#pragma once
#include <stdint.h>

#include "../../include/nabo_bundle.h"

namespace nabo {

struct BundleView {
    int device;
    int64_t n_edges, n_points;
    const int64_t *off;   // device, [n_edges + 1]
    const double *pts;    // device, [n_points][2], normalised
    double lo[2], span[2];
};

BundleView bundle_view(const nabo_bundle *B);

}  // namespace nabo
