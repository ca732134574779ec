"""Brute-force fp64 numpy oracle of gdrnet_amd.shade (gdrn_render_visibility, gdrn_shade_frames; the rules: include/gdrn_hip.h): every pixel
against every triangle through the rules of tests/render_host.py, then the reference's lighting per pixel.  GL cannot run where this project is
built and tested and the reference's lighting exists only as shader text, so this file restates it:

  shader/depth_shader_phong.vs:93-94     P = view * position, v_view = -P              -> V = normalize(-P)
  shader/depth_shader_phong.vs:101       v_L = normalize(u_light_eye_pos - P)          -> L = normalize(light - P)
  shader/depth_shader_phong.vs:102       v_normal: the normal in eye coordinates       -> N = normalize(R n)  (the 4-vector normalisation is not reproduced)
  shader/depth_shader_phong.frag:20-22   Normal, LightDir, ViewDir normalised
  shader/depth_shader_phong.frag:24      diffuse = max(dot(Normal, LightDir), 0) * v_color
  shader/depth_shader_phong.frag:25-26   R = reflect(-LightDir, Normal) = 2 (N.L) N - L;  specular = max(dot(R, ViewDir), 0) * v_color  (no gate on N.L)
  shader/depth_shader_phong.frag:29-35   rgb = ambient v_color + diffuse_w diffuse + specular_w specular, clamped at 1 per channel
  shader/depth_shader_phong.frag:36      rgb_normals = Normal * 0.5 + 0.5
  meshrenderer_phong.py:136,162          the weights (0.4, 0.8, 0.3) and the light at GL eye (400, 400, 400) mm

Light and view vectors are evaluated PER PIXEL at P = z d (z = (n.a) / (n.d) in fp64), colour and normal interpolated perspective-correctly with
the weights d.(b x c), d.(c x a), d.(a x b) over their sum; bytes are floor(255 v + 0.5)."""
import numpy as np

import render_host as RH


def vertex_normals(v, f):
    """area-weighted vertex normals written as a plain loop over the faces (shares nothing with gdrnet_amd.shade.vertex_normals)"""
    v = np.asarray(v, dtype=np.float64)
    acc = np.zeros_like(v)
    for a, b, c in np.asarray(f, dtype=np.int64):
        n = np.cross(v[b] - v[a], v[c] - v[a])
        acc[a] += n
        acc[b] += n
        acc[c] += n
    return acc / np.linalg.norm(acc, axis=1, keepdims=True)


def colors_f64(col):
    col = np.asarray(col)
    return col.astype(np.float64) / 255.0 if col.dtype == np.uint8 else col.astype(np.float64)


def _posed(verts, faces, R, t):
    """camera-space vertices a, b, c [T,3] of every face, vertex indices sorted ascending; the sorted faces"""
    fs = np.sort(np.asarray(faces, dtype=np.int64), axis=1)
    vc = np.asarray(verts, dtype=np.float64) @ np.asarray(R, dtype=np.float64).T + np.asarray(t, dtype=np.float64)
    return vc[fs[:, 0]], vc[fs[:, 1]], vc[fs[:, 2]], fs


def fragments(verts, faces, R, t, K, H, W, near=0.01, far=6.5):
    """every fragment the rules of gdrn_render_depth keep, sorted by (pixel, fp32 depth, face index): (pixel [M], face [M], zf [M] fp32)"""
    a, b, c, _ = _posed(verts, faces, R, t)
    n = np.cross(b - a, c - a)
    keep = np.flatnonzero((a[:, 2] >= near) & (b[:, 2] >= near) & (c[:, 2] >= near) & np.any(n != 0, axis=1))
    dx, dy = RH.pixel_rays(K, H, W)
    D = np.stack([dx, dy, np.ones_like(dx)], axis=0)
    pix, fac, zfs = [], [], []
    for s in range(0, len(keep), RH.CHUNK):
        k = keep[s : s + RH.CHUNK]
        E = np.stack([np.cross(a[k], b[k]), np.cross(b[k], c[k]), -np.cross(a[k], c[k])], axis=1)
        w = np.einsum("tek,kp->tep", E, D)
        ti, pi = np.nonzero(np.all(w >= 0, axis=1) | np.all(w <= 0, axis=1))
        nk = n[k][ti]
        den = nk[:, 0] * dx[pi] + (nk[:, 1] * dy[pi] + nk[:, 2])
        ok = den != 0
        ti, pi, nk, den = ti[ok], pi[ok], nk[ok], den[ok]
        z = np.einsum("ij,ij->i", nk, a[k][ti]) / den
        with np.errstate(over="ignore"):
            zf = z.astype(np.float32)
        ok = ~(z > far) & (zf > 0) & np.isfinite(zf)
        pix.append(pi[ok])
        fac.append(k[ti[ok]])
        zfs.append(zf[ok])
    pix, fac, zfs = (np.concatenate(x) if x else np.zeros(0, dt) for x, dt in ((pix, np.int64), (fac, np.int64), (zfs, np.float32)))
    order = np.lexsort((fac, zfs, pix))
    return pix[order], fac[order], zfs[order]


def visibility_one(verts, faces, R, t, K, H, W, near=0.01, far=6.5):
    """(depth [H*W] fp32 with 0 = nothing, face [H*W] int64 with -1 = nothing, second [H*W] fp32: the depth of the pixel's second fragment in
    (depth, face) order, +inf without one, frags: the sorted fragment arrays): the winner is the nearest fp32 depth, the lowest face index among equals"""
    pix, fac, zf = fragments(verts, faces, R, t, K, H, W, near, far)
    depth, face, second = np.zeros(H * W, np.float32), np.full(H * W, -1, np.int64), np.full(H * W, np.inf, np.float32)
    first = np.flatnonzero(np.r_[True, pix[1:] != pix[:-1]]) if len(pix) else np.zeros(0, np.int64)
    depth[pix[first]], face[pix[first]] = zf[first], fac[first]
    nxt = first + 1
    has = nxt < len(pix)
    has[has] &= pix[nxt[has]] == pix[first[has]]
    second[pix[first[has]]] = zf[nxt[has]]
    return depth, face, second, (pix, fac, zf)


def fragment_depth(frags, nfaces, pixel, face):
    """the fp32 depth of the fragments (pixel[k], face[k]), NaN where the face does not cover the pixel"""
    pix, fac, zf = frags
    key = pix * nfaces + fac
    order = np.argsort(key)
    want = np.asarray(pixel, dtype=np.int64) * nfaces + np.asarray(face, dtype=np.int64)
    pos = np.clip(np.searchsorted(key[order], want), 0, max(len(key) - 1, 0))
    out = np.full(len(want), np.nan, dtype=np.float32)
    if len(key):
        hit = key[order][pos] == want
        out[hit] = zf[order][pos[hit]]
    return out


def _unit(v):
    l = np.linalg.norm(v, axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(l > 0, v / l, 0.0)


def shade_values(verts, faces, colors, normals, R, t, K, H, W, light, phong, pixel, face, affine=False):
    """(rgb [M,3], normal map [M,3]) as fp64 values in [0, 1] -- before the quantisation -- of the pixels `pixel` (flat indices) shaded as face
    `face[k]` of the mesh under (R, t).  `affine`: interpolate with screen-space barycentrics of the projected vertices instead (what the CPU test
    shows to be distinguishable from the rule)."""
    a, b, c, fs = _posed(verts, faces, R, t)
    face = np.asarray(face, dtype=np.int64)
    a, b, c, fs = a[face], b[face], c[face], fs[face]
    dx, dy = RH.pixel_rays(K, H, W)
    d = np.stack([dx[pixel], dy[pixel], np.ones(len(face))], axis=1)
    n = np.cross(b - a, c - a)
    z = np.einsum("ij,ij->i", n, a) / np.einsum("ij,ij->i", n, d)
    P = z[:, None] * d
    w = np.stack([np.einsum("ij,ij->i", d, np.cross(b, c)), np.einsum("ij,ij->i", d, np.cross(c, a)), np.einsum("ij,ij->i", d, np.cross(a, b))], axis=1)
    if affine:
        Kd = np.asarray(K, dtype=np.float64)
        pr = [(v @ Kd.T)[:, :2] / v[:, 2:3] for v in (a, b, c)]
        y, x = np.divmod(np.asarray(pixel), W)
        q = np.stack([x, y], axis=1).astype(np.float64)
        ar = lambda p0, p1, p2: (p1[:, 0] - p0[:, 0]) * (p2[:, 1] - p0[:, 1]) - (p1[:, 1] - p0[:, 1]) * (p2[:, 0] - p0[:, 0])  # noqa: E731
        w = np.stack([ar(q, pr[1], pr[2]), ar(q, pr[2], pr[0]), ar(q, pr[0], pr[1])], axis=1)
    w = w / w.sum(axis=1, keepdims=True)
    col, nrm = colors_f64(colors), np.asarray(normals, dtype=np.float64)
    ci = sum(w[:, k : k + 1] * col[fs[:, k]] for k in range(3))
    ni = sum(w[:, k : k + 1] * nrm[fs[:, k]] for k in range(3))
    N = _unit(ni @ np.asarray(R, dtype=np.float64).T)
    L = _unit(np.asarray(light, dtype=np.float64)[None] - P)
    V = _unit(-P)
    nl = np.einsum("ij,ij->i", N, L)
    diff = np.maximum(nl, 0.0)
    Rv = 2.0 * nl[:, None] * N - L
    spec = np.maximum(np.einsum("ij,ij->i", Rv, V), 0.0)
    amb, dif, spe = (float(x) for x in phong)
    rgb = np.minimum(1.0, (amb + dif * diff + spe * spec)[:, None] * ci)
    return rgb, 0.5 * N + 0.5


def quantise(v):
    return np.floor(255.0 * v + 0.5).astype(np.uint8)


class Scene:
    """The oracle's view of a synth.make_shade_inputs scene: per instance the visibility (depth, face, second, frags), the vertex normals per class,
    and the frames composed by the rules (nearest fp32 depth, first in input order among equals)."""

    def __init__(self, inp, stats=None):
        self.inp = inp
        self.H, self.W, self.F = inp["H"], inp["W"], inp["num_frames"]
        self.normals = [vertex_normals(v, f) for v, f in zip(inp["vertices"], inp["faces"])]
        self.inst = []
        for i, c in enumerate(inp["labels"]):
            self.inst.append(visibility_one(inp["vertices"][c], inp["faces"][c], inp["R"][i], inp["t"][i], inp["K"][i], self.H, self.W, inp["near"], inp["far"]))
        if stats is not None:
            RH.render_depth(inp, stats)
        HW = self.H * self.W
        self.depth, self.index, self.face = np.zeros((self.F, HW), np.float32), np.full((self.F, HW), -1, np.int64), np.full((self.F, HW), -1, np.int64)
        for i, f in enumerate(inp["frame"]):
            d, fc = self.inst[i][0], self.inst[i][1]
            take = (d != 0) & ((self.depth[f] == 0) | (d < self.depth[f]))   # strict: the earlier instance keeps a tie
            self.depth[f][take], self.index[f][take], self.face[f][take] = d[take], i, fc[take]

    def values(self, f, pixel, index, face, affine=False):
        """(rgb, normal map) fp64 values of frame f's pixels `pixel`, shaded as face `face[k]` of instance `index[k]`"""
        inp = self.inp
        rgb, nrm = np.zeros((len(pixel), 3)), np.zeros((len(pixel), 3))
        for i in np.unique(index):
            m, c = index == i, inp["labels"][i]
            rgb[m], nrm[m] = shade_values(inp["vertices"][c], inp["faces"][c], inp["colors"][c], self.normals[c], inp["R"][i], inp["t"][i], inp["K"][i],
                                          self.H, self.W, inp["light"][f], inp["phong"][f], pixel[m], face[m], affine)
        return rgb, nrm

    def frames(self, background=True, affine=False):
        """(rgb [F,H,W,3] u8, values [F,H*W,3] fp64 with NaN where nothing is drawn) by the oracle's own winners"""
        H, W, F = self.H, self.W, self.F
        out = self.inp["background"].reshape(F, H * W, 3).copy() if background else np.zeros((F, H * W, 3), np.uint8)
        vals = np.full((F, H * W, 3), np.nan)
        for f in range(F):
            pixel = np.flatnonzero(self.index[f] >= 0)
            if len(pixel):
                vals[f, pixel] = self.values(f, pixel, self.index[f][pixel], self.face[f][pixel], affine)[0]
                out[f, pixel] = quantise(vals[f, pixel])
        return out.reshape(F, H, W, 3), vals
