// misc.depth_im_to_dist_im_fast (lib/pysixd/misc.py:565-588) for one pixel, shared by bop_metrics.hip (VSD) and scene_gt.hip (ground-truth visibility):
// sqrt((X d)^2 + (Y d)^2 + d^2) with X = (x - cx) / fx, Y = (y - cy) / fy, every operation a separate fp64 operation as numpy evaluates it.
// Floating-point contraction is switched off INSIDE the function, so the bits do not depend on where the including file puts its own pragma.
#pragma once

namespace {

__device__ __forceinline__ double dist_of(double X, double Y, float depth) {
#pragma clang fp contract(off)
    const double d = (double)depth, a = X * d, b = Y * d;
    return sqrt((a * a + b * b) + d * d);
}

}  // namespace
