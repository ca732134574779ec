"""fp64 numpy oracle of gdrnet_amd.shade.render_frames_bop (gdrn_shade_frames_tex; the rules: include/gdrn_hip.h): coverage, winner and face come
from tests/shade_host.py (SH.Scene, unchanged), this file adds what the BOP renderer lib/pysixd/renderer_py.py does per pixel.  GL cannot run where
this project is built and tested, so the rules are restated from the header, not taken from the reference's shader text:

  uv          perspective-correct, with the weights d.(b x c), d.(c x a), d.(a x b) over their sum (vertex indices sorted ascending)
  normal      "phong": normalize(R n_interp);  "flat": normalize((b - a) x (c - a)) in camera space, negated when it points away from the camera
  light       L = normalize(light - P);  lw = min(1, ambient + max(N.L, 0));  no specular term
  base colour the texture at uv where the class has one (v = 0 is the bottom row of the image, clamp-to-edge, nearest or bilinear), else the
              interpolated vertex colour; a class without colours is 0.5 gray
  bytes       np.round(255 lw c): half to even"""
import numpy as np

import render_host as RH
import shade_host as SH

GRAY = 0.5
NEAR_INT = 1e-9   # a pixel whose u w or v h is this close to an integer may take the neighbouring texel on the device (nearest sampling)


def sample_nearest(texture, u, v):
    """[M,3] fp64 in [0, 1]: the texel under (u, v) of a [h,w,3] u8 image in file row order"""
    h, w = texture.shape[:2]
    i = np.clip(np.floor(u * w), 0, w - 1).astype(np.int64)
    j = np.clip(np.floor(v * h), 0, h - 1).astype(np.int64)
    return texture[h - 1 - j, i].astype(np.float64) / 255.0


def sample_bilinear(texture, u, v):
    """[M,3] fp64: the four texels round (u w - 0.5, v h - 0.5), clamped to the edge, blended along x and then along y"""
    h, w = texture.shape[:2]
    up = texture[::-1].astype(np.float64)   # row j of `up` is the j-th row from the bottom
    x, y = u * w - 0.5, v * h - 0.5
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf)[:, None], (y - yf)[:, None]
    i0, i1 = np.clip(xf, 0, w - 1).astype(np.int64), np.clip(xf + 1, 0, w - 1).astype(np.int64)
    j0, j1 = np.clip(yf, 0, h - 1).astype(np.int64), np.clip(yf + 1, 0, h - 1).astype(np.int64)
    lo = up[j0, i0] + fx * (up[j0, i1] - up[j0, i0])
    hi = up[j1, i0] + fx * (up[j1, i1] - up[j1, i0])
    return (lo + fy * (hi - lo)) / 255.0


def pixel_geometry(verts, faces, R, t, K, H, W, pixel, face):
    """of the pixels `pixel` (flat indices) seen as face `face[k]` of the mesh under (R, t): dict(fs [M,3] sorted vertex indices, w [M,3] the
    normalised weights of those vertices, n [M,3] the camera-space face normal (b - a) x (c - a), d [M,3] the ray, P [M,3] the surface point)"""
    a, b, c, fs = SH._posed(verts, faces, R, t)
    face = np.asarray(face, dtype=np.int64)
    a, b, c, fs = a[face], b[face], c[face], fs[face]
    dx, dy = RH.pixel_rays(K, H, W)
    d = np.stack([dx[pixel], dy[pixel], np.ones(len(face))], axis=1)
    n = np.cross(b - a, c - a)
    z = np.einsum("ij,ij->i", n, a) / np.einsum("ij,ij->i", n, d)
    w = np.stack([np.einsum("ij,ij->i", d, np.cross(b, c)), np.einsum("ij,ij->i", d, np.cross(c, a)), np.einsum("ij,ij->i", d, np.cross(a, b))], axis=1)
    return dict(fs=fs, w=w / w.sum(axis=1, keepdims=True), n=n, d=d, P=z[:, None] * d)


def tex_values(verts, faces, colors, normals, uv, texture, R, t, K, H, W, light, ambient, pixel, face, shading="phong", filter="nearest"):
    """dict(rgb [M,3], nmap [M,3]: fp64 values in [0, 1] before the quantisation; N [M,3] the normal used; lw [M]; uv [M,2] (NaN without a
    texture); dist [M]: the smaller distance of u w and v h to an integer, +inf without a texture)"""
    g = pixel_geometry(verts, faces, R, t, K, H, W, pixel, face)
    fs, w = g["fs"], g["w"]
    interp = lambda tab: sum(w[:, k : k + 1] * np.asarray(tab, dtype=np.float64)[fs[:, k]] for k in range(3))  # noqa: E731
    if shading == "flat":
        N = SH._unit(g["n"])
        N = np.where(np.einsum("ij,ij->i", g["n"], g["d"])[:, None] > 0, -N, N)
    else:
        N = SH._unit(interp(normals) @ np.asarray(R, dtype=np.float64).T)
    L = SH._unit(np.asarray(light, dtype=np.float64)[None] - g["P"])
    lw = np.minimum(1.0, float(ambient) + np.maximum(np.einsum("ij,ij->i", N, L), 0.0))
    M = len(fs)
    uvp, dist = np.full((M, 2), np.nan), np.full(M, np.inf)
    if texture is not None:
        uvp = interp(uv)
        h, wd = texture.shape[:2]
        s = np.stack([uvp[:, 0] * wd, uvp[:, 1] * h], axis=1)
        dist = np.abs(s - np.round(s)).min(axis=1)
        base = (sample_nearest if filter == "nearest" else sample_bilinear)(texture, uvp[:, 0], uvp[:, 1])
    else:
        base = np.full((M, 3), GRAY) if colors is None else interp(SH.colors_f64(colors))
    return dict(rgb=lw[:, None] * base, nmap=0.5 * N + 0.5, N=N, lw=lw, uv=uvp, dist=dist)


def quantise(v):
    return np.clip(np.round(255.0 * v), 0, 255).astype(np.uint8)


class TexScene(SH.Scene):
    """SH.Scene (visibility per instance, the composed depth / index / face) of a synth.make_tex_inputs scene, shaded by the rules above"""

    def values(self, f, pixel, index, face, shading="phong", filter="nearest"):
        """(rgb [M,3], normal map [M,3], dist [M]) of frame f's pixels `pixel`, shaded as face `face[k]` of instance `index[k]`"""
        inp = self.inp
        rgb, nrm, dist = np.zeros((len(pixel), 3)), np.zeros((len(pixel), 3)), np.full(len(pixel), np.inf)
        for i in np.unique(index):
            m, c = index == i, inp["labels"][i]
            r = tex_values(inp["vertices"][c], inp["faces"][c], inp["colors"][c], self.normals[c], inp["uvs"][c], inp["textures"][c], inp["R"][i],
                           inp["t"][i], inp["K"][i], self.H, self.W, inp["light"][f], inp["ambient"][f], pixel[m], face[m], shading, filter)
            rgb[m], nrm[m], dist[m] = r["rgb"], r["nmap"], r["dist"]
        return rgb, nrm, dist

    def frames(self, shading="phong", filter="nearest", background=True):
        """(rgb [F,H,W,3] u8, values [F,H*W,3] fp64 with NaN where nothing is drawn, dist [F,H*W] with +inf where no texture is sampled) by the
        oracle's own winners"""
        H, W, F = self.H, self.W, self.F
        out = self.inp["background"].reshape(F, H * W, 3).copy() if background else np.zeros((F, H * W, 3), np.uint8)
        vals, dist = np.full((F, H * W, 3), np.nan), np.full((F, H * W), np.inf)
        for f in range(F):
            pixel = np.flatnonzero(self.index[f] >= 0)
            if len(pixel):
                vals[f, pixel], _, dist[f, pixel] = self.values(f, pixel, self.index[f][pixel], self.face[f][pixel], shading, filter)
                out[f, pixel] = quantise(vals[f, pixel])
        return out.reshape(F, H, W, 3), vals, dist
