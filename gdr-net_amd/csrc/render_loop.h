// The arguments of a render as one value, and the host rules of the loops that render per iteration (gdrn_icp_refine, gdrn_icp_refine_sil,
// gdrn_depth_align): each of them starts with gdrn_render_depth's own list, with the scene and the frame of every row behind N.  The first
// part (RenderRows, rows_*) also holds the rasterizer's own rules: csrc/render.hip's raster_args reads them and uses nothing below them.
// Host code only; included behind geom64.h (host_in_range) and include/gdrn_hip.h.
#pragma once

namespace {

// the mesh table and the rows drawn from it: gdrn_render_depth's arguments up to the output
struct RenderRows {
    const double* verts;
    const int *faces, *vert_off, *nverts, *face_off, *nfaces;
    int C, f_max;
    const int *labels, *labels_host;
    const double *R, *t, *K;
    int N, H, W;
    double near, far;
};

// the observed frames and the frame of every row
struct RenderScene {
    const float* depth_scene;
    const int *frame, *frame_host;
    int F;
};

inline bool rows_scalars_ok(const RenderRows& a) { return a.C > 0 && a.f_max > 0 && a.near > 0.0 && a.near < a.far; }
inline bool rows_pointers_ok(const RenderRows& a) {
    return a.verts && a.faces && a.vert_off && a.nverts && a.face_off && a.nfaces && a.labels && a.labels_host && a.R && a.t && a.K;
}

// The checks of a loop, in two parts around its `N == 0` return.  Before it: the scalars all loops judge alike (the frame limit and the gates
// are the loop's own).  Behind it, and behind the loop's own pointers: the shared pointers, the grid limit of the instances, the host ranges.
inline bool loop_scalars_ok(const RenderRows& a, const RenderScene& s) { return s.F >= 0 && rows_scalars_ok(a); }
inline int loop_rows_check(const RenderRows& a, const RenderScene& s) {
    if (!rows_pointers_ok(a) || !s.depth_scene || !s.frame || !s.frame_host) return GDRN_ERR_ARG;
    if (a.N > 65535) return GDRN_ERR_SHAPE;   // the instances are the grid's second dimension
    if (!host_in_range(a.labels_host, a.N, a.C) || !host_in_range(s.frame_host, a.N, s.F)) return GDRN_ERR_ARG;
    return GDRN_OK;
}

// the rows under their current poses into depth [N][H][W]
inline int render_into(const RenderRows& a, float* depth, void* stream) {
    return gdrn_render_depth(a.verts, a.faces, a.vert_off, a.nverts, a.face_off, a.nfaces, a.C, a.f_max, a.labels, a.labels_host, a.R, a.t, a.K,
                             a.N, a.H, a.W, a.near, a.far, depth, stream);
}

}  // namespace
