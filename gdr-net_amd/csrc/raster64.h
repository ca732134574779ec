// What the rasterizer (render.hip) and the shading pass (shade.hip) share: the camera, the pixel's ray and the cross product -- one definition, so
// that the shading pass repeats the rasterizer's ray and edge values operation by operation.  Include after geom64.h and BEHIND
// `#pragma clang fp contract(off)`: the products and differences here must not be fused.
#pragma once

namespace {

struct Cam { double fx, sk, cx, fy, cy; };      // K = [[fx, sk, cx], [0, fy, cy], [0, 0, 1]]

__device__ __forceinline__ Cam load_cam(const double* K) { return Cam{K[0], K[1], K[2], K[4], K[5]}; }

__device__ __forceinline__ V3 cross(V3 p, V3 q) {
    return V3{p.y * q.z - p.z * q.y, p.z * q.x - p.x * q.z, p.x * q.y - p.y * q.x};
}

// the ray of pixel (x, y): K^-1 [x, y, 1] for the upper-triangular K, third component exactly 1
__device__ __forceinline__ void pixel_ray(const Cam& c, int x, int y, double& dx, double& dy) {
    dy = ((double)y - c.cy) / c.fy;
    dx = (((double)x - c.sk * dy) - c.cx) / c.fx;
}

}  // namespace
