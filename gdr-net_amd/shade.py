"""Shaded colour renders of posed meshes into frames on the device (csrc/shade.hip, the visibility pass of csrc/render.hip).

Device-side counterpart of the reference's GL renderer ``lib/meshrenderer/meshrenderer_phong.py`` (``render``, ``render_many``) with
``shader/depth_shader_phong.{vs,frag}``: vertex-colour Phong shading and a z-test between several posed objects in one image -- the renderer
behind the xyz tool and the pose visualisation of ``core/utils/pose_utils.py``, and the usual way to rendered-object-over-background frames.
Two passes: ``render_visibility`` runs the depth rasterizer's walk with 64-bit keys (fp32 depth bits above the face index), ``render_frames``
picks the nearest instance per frame pixel, recomputes that face's geometry in fp64 and shades it.  The rules are stated with the entry points
in ``include/gdrn_hip.h``; what differs from the GL renderer is listed in INTEGRATION.md.  There is no CPU fallback.
``render_frames_bop`` is the same render with the light model of the reference's second renderer, ``lib/pysixd/renderer_py.py`` (behind
``renderer.create_renderer(..., mode="rgb")``): a UV texture map per class (``TexturedMeshTable``) instead of vertex colours where a model has
one, Phong or flat shading, ``min(1, ambient + max(N.L, 0))`` without a specular term, bytes rounded half to even.

Conventions: camera coordinates are OpenCV's (x right, y down, z forward), metres.  The reference's light is a position in GL eye space
(x right, y up, z backward) for models in millimetres; ``from_gl_eye_mm`` converts.
"""
import numpy as np
import torch

from . import cabi, devargs, render
from .scene_gt import csr_of_frames

WHERE = "the shaded renderer"   # (this module in devargs' error sentence)
PHONG = (0.4, 0.8, 0.3)         # ambient, diffuse, specular: meshrenderer_phong.py:136
LIGHT = (0.4, -0.4, -0.4)       # the reference's GL eye-space (400, 400, 400) mm (meshrenderer_phong.py:162) in this project's convention


def from_gl_eye_mm(p):
    """a position in GL eye space, millimetres -> this project's camera coordinates, metres: (x, -y, -z) / 1000"""
    return np.asarray(p, dtype=np.float64) * np.array([1e-3, -1e-3, -1e-3])


def vertex_normals(vertices, faces):
    """Unit vertex normals [n,3] fp64 of a triangle mesh, host numpy, computed once per dataset: per vertex the sum of ``(b - a) x (c - a)`` over the
    faces (a, b, c) it belongs to -- each face weighted by its area -- normalised.  The orientation FOLLOWS THE WINDING: counter-clockwise faces
    seen from outside give outward normals; a mesh with mixed windings gives normals that partly cancel.  A vertex that belongs to no face, or
    whose sum is zero, raises ValueError."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"face index outside [0, {len(v)})")
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    acc = np.zeros_like(v)
    for k in range(3):
        np.add.at(acc, f[:, k], fn)
    used = np.zeros(len(v), dtype=bool)
    used[f.ravel()] = True
    length = np.linalg.norm(acc, axis=1)
    if not used.all():
        raise ValueError(f"vertex {int(np.flatnonzero(~used)[0])} belongs to no face: it has no normal")
    if not np.all(np.isfinite(length)) or np.any(length == 0):
        raise ValueError(f"vertex {int(np.flatnonzero(~(length > 0))[0])}: the face normals round it sum to zero")
    return acc / length[:, None]


class ShadedMeshTable(render.MeshTable):
    """A ``render.MeshTable`` with per-vertex colours and unit normals (``colors`` / ``normals``, fp64, packed like ``verts``): everything that
    takes a MeshTable (``render.render_depth``, ``scene_gt``, ``bop_metrics.vsd``) takes it unchanged.  ``colors_list``: per class [n_c,3], u8
    (divided by 255 in fp64) or floats in [0, 1], in any channel order -- ``render_frames`` writes the same order.  ``normals_list``: per class
    [n_c,3] in model coordinates, normalised here in fp64; ``None`` (for the list or for one class): ``vertex_normals``.  Anything non-finite, a
    colour outside [0, 1] or a zero normal raises ValueError."""

    TABLES = render.MeshTable.TABLES + ("normals", "colors")

    def __init__(self, vertices_list, faces_list, colors_list, normals_list=None, device=None):
        super().__init__(vertices_list, faces_list)
        C = self.num_classes
        if len(colors_list) != C or (normals_list is not None and len(normals_list) != C):
            raise ValueError("colors_list and normals_list need one entry per class")
        if not np.all(np.isfinite(self.verts)):
            raise ValueError("vertices must be finite")
        cols, nrms = [], []
        for c in range(C):
            n = int(self.nverts[c])
            col = np.asarray(colors_list[c])
            if col.dtype == np.uint8:
                col = col.astype(np.float64) / 255.0
            elif np.issubdtype(col.dtype, np.floating):
                col = col.astype(np.float64)
            else:
                raise ValueError(f"colours of class {c}: u8 or floats in [0, 1]")
            if col.shape != (n, 3):
                raise ValueError(f"colours of class {c}: [{n}, 3], one per vertex")
            if not np.all(np.isfinite(col)) or col.min() < 0.0 or col.max() > 1.0:
                raise ValueError(f"colours of class {c} outside [0, 1]")
            cols.append(col)
            v0, f0 = int(self.vert_off[c]), int(self.face_off[c])
            given = None if normals_list is None else normals_list[c]
            if given is None:
                nrm = vertex_normals(self.verts[v0 : v0 + n], self.faces[f0 : f0 + int(self.nfaces[c])])
            else:
                nrm = np.asarray(given, dtype=np.float64)
                if nrm.shape != (n, 3):
                    raise ValueError(f"normals of class {c}: [{n}, 3], one per vertex")
                length = np.linalg.norm(nrm, axis=1)
                if not np.all(np.isfinite(nrm)) or not np.all(np.isfinite(length)) or np.any(length == 0):
                    raise ValueError(f"normals of class {c}: finite and not zero")
                nrm = nrm / length[:, None]
            nrms.append(nrm)
        self.colors = np.ascontiguousarray(np.concatenate(cols, axis=0))
        self.normals = np.ascontiguousarray(np.concatenate(nrms, axis=0))
        if device is not None:
            self.on(device)


def render_visibility(table, labels, R, t, K, H, W, near=render.NEAR, far=render.FAR):
    """Visibility keys [N,H,W] int64 (bit patterns) of N instances, arguments and rules as ``render.render_depth``: the bits of the fp32 depth
    above the index of the face (within its class) that wins the pixel -- the nearest fp32 depth, the lowest face index among equal depths;
    all ones (-1) where nothing is drawn.  ``visibility_depth`` / ``visibility_face`` give the two halves."""
    R, t, K, N = devargs.poses(R, t, K, WHERE)
    dev = R.device
    lab, lab_host = devargs.index_vector(labels, N, table.num_classes, dev, "labels")
    H, W = int(H), int(W)
    vis = torch.empty(max(N, 0), max(H, 0), max(W, 0), dtype=torch.int64, device=dev)
    if N == 0:
        return vis
    p = cabi.ptr
    cabi.check(cabi.load().gdrn_render_visibility(*table.lib_args(dev), p(lab), lab_host.ctypes.data, p(R), p(t), p(K), N, H, W, float(near),
                                                  float(far), p(vis), devargs.stream(dev)), "render_visibility")
    return vis


def visibility_depth(vis):
    """the depth [N,H,W] fp32 of visibility keys: what ``render.render_depth`` returns for the same inputs, bit for bit (0 where nothing is drawn)"""
    bits = (vis >> 32).to(torch.int32)   # (arithmetic shift: the low 32 bits of the result are the key's upper half)
    return torch.where(vis == -1, torch.zeros_like(bits), bits).view(torch.float32)


def visibility_face(vis):
    """the winning face [N,H,W] int32 of visibility keys, -1 where nothing is drawn"""
    return (vis & 0xFFFFFFFF).to(torch.int32)   # (the empty key's lower half is all ones: -1)


class Frames:
    """The result of ``render_frames``, device tensors: ``rgb`` [F,H,W,3] u8 (channel order of the colour table); ``depth`` [F,H,W] fp32, 0 where
    nothing is drawn; ``index`` [F,H,W] int32, the row of the instance that owns the pixel, -1 where nothing is drawn; ``face`` [F,H,W] int32 and
    ``normals`` [F,H,W,3] u8 when asked for, else None; ``vis`` [N,H,W] int64, the visibility keys of the instances."""

    def __init__(self, rgb, depth, index, face, normals, vis):
        self.rgb, self.depth, self.index, self.face, self.normals, self.vis = rgb, depth, index, face, normals, vis


def _per_frame(values, F, what, nonneg):
    """[F,3] fp64 host array from [3] or [F,3] (host values or a tensor), finite (and >= 0 with `nonneg`): ValueError otherwise"""
    a = values.detach().cpu().numpy() if isinstance(values, torch.Tensor) else np.asarray(values)
    try:
        a = a.astype(np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: [3] or [F, 3] numbers") from None
    if a.shape == (3,):
        a = np.broadcast_to(a, (F, 3))
    if a.shape != (F, 3):
        raise ValueError(f"{what}: [3] or [{F}, 3]")
    if not np.all(np.isfinite(a)) or (nonneg and a.size and a.min() < 0.0):
        raise ValueError(f"{what}: finite" + (" and not negative" if nonneg else ""))
    return np.ascontiguousarray(a)




def _render(table, labels, R, t, K, H, W, frame, num_frames, light, weights, background, want_face, want_normals, near, far, launch):
    """The two-pass render behind ``render_frames`` and ``render_frames_bop``: argument checks, the visibility pass, the outputs, the CSR table and
    the side tables.  ``weights(F)``: the per-frame fp64 host array that follows the lights in the fp64 side table.  ``launch(dev, vis, mesh, inst,
    maps)`` makes the C call from the pointer groups of the shade entry points: the keys | verts .. colors | C .. W, light, weights | background .. stream."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("H and W: at least one pixel")
    R, t, K, N = devargs.poses(R, t, K, WHERE)
    dev = R.device
    lab, lab_host = devargs.index_vector(labels, N, table.num_classes, dev, "labels")
    if num_frames is None:
        fr_host = devargs.index_vector(frame, N, None, dev, "frame")[1]
        if fr_host.size and fr_host.min() < 0:
            raise ValueError("frame outside [0, F)")
        F = int(fr_host.max()) + 1 if fr_host.size else 0
    else:
        F = int(num_frames)
        if F < 0:
            raise ValueError("num_frames: not negative")
        fr_host = devargs.index_vector(frame, N, F, dev, "frame")[1]
    light, weights = _per_frame(light, F, "light", False), weights(F)
    if background is not None:
        background = devargs.device_tensor(background, None, None, "background", WHERE)
        if background.dtype != torch.uint8 or tuple(background.shape) != (F, H, W, 3):
            raise ValueError(f"background must be u8 [{F}, {H}, {W}, 3]")
        if background.data_ptr() % 4:
            background = background.clone()   # (a view at an odd offset: the kernel reads aligned dwords)
    vis = render_visibility(table, lab_host, R, t, K, H, W, near, far)
    u8 = dict(dtype=torch.uint8, device=dev)
    out = Frames(torch.empty(F, H, W, 3, **u8), torch.empty(F, H, W, dtype=torch.float32, device=dev),
                 torch.empty(F, H, W, dtype=torch.int32, device=dev), torch.empty(F, H, W, dtype=torch.int32, device=dev) if want_face else None,
                 torch.empty(F, H, W, 3, **u8) if want_normals else None, vis)
    if F == 0:
        return out
    off_host, inst_host = csr_of_frames(fr_host, F)
    ints = torch.from_numpy(np.concatenate([off_host, inst_host])).to(dev)                # one upload each of the integer
    reals = torch.from_numpy(np.concatenate([light.ravel(), weights.ravel()])).to(dev)    # and the fp64 side tables
    tb, p = table.on(dev), cabi.ptr
    mesh = [p(tb[k]) for k in ("verts", "faces", "vert_off", "nverts", "face_off", "nfaces", "normals", "colors")]
    inst = (table.num_classes, p(lab), lab_host.ctypes.data, p(R), p(t), p(K), p(ints), off_host.ctypes.data, p(ints[F + 1:]), inst_host.ctypes.data,
            F, N, H, W, p(reals), p(reals[3 * F:]))
    maps = (p(background), p(out.rgb), p(out.depth), p(out.index), p(out.face), p(out.normals), devargs.stream(dev))
    launch(dev, p(vis), mesh, inst, maps)
    return out


def render_frames(table, labels, R, t, K, H, W, frame, num_frames=None, light=LIGHT, phong=PHONG, background=None, want_face=False,
                  want_normals=False, near=render.NEAR, far=render.FAR):
    """Shaded frames of N posed instances: instance i is the mesh ``labels[i]`` of the ``ShadedMeshTable`` ``table`` under ``R[i]``, ``t[i]`` seen
    through ``K[i]`` ([3,3]: shared) in frame ``frame[i]`` -- poses and K device tensors as ``render.render_depth`` takes them, ``labels`` and
    ``frame`` [N] from the host or the device, checked on the host.  ``num_frames``: F (default max(frame) + 1); a frame without instances is
    its background.  ``light`` [3] or [F,3]: the light's position in camera coordinates, metres; ``phong`` [3] or [F,3]: (ambient, diffuse,
    specular), finite and >= 0.  ``background`` [F,H,W,3] u8 device tensor or None (black).  Per pixel the nearest instance wins (the first in
    input order among equal fp32 depths).  Returns a ``Frames``; nothing is read back."""
    if not isinstance(table, ShadedMeshTable):
        raise ValueError("render_frames needs a ShadedMeshTable (colours and normals per vertex)")

    def launch(dev, vis, mesh, inst, maps):
        cabi.check(cabi.load().gdrn_shade_frames(vis, *mesh, *inst, *maps), "shade_frames")

    return _render(table, labels, R, t, K, H, W, frame, num_frames, light, lambda F: _per_frame(phong, F, "phong", True), background, want_face,
                   want_normals, near, far, launch)


# ---- the BOP renderer's light model: UV textures, flat shading (lib/pysixd/renderer_py.py) ----
AMBIENT = 0.5                # renderer.py:24-28: the default ambient weight; the default light sits at the camera origin
GRAY = 0.5                   # a model without colours is drawn gray (renderer_py.py:348-350)
TEX_MAX_SIDE = 16384         # GDRN_TEX_MAX_SIDE
SHADINGS = {"phong": 0, "flat": 1}         # GDRN_SHADING_*
FILTERS = {"nearest": 0, "bilinear": 1}    # GDRN_TEXFILTER_*


def pack_texels(image):
    """[h,w,3] u8 -> [h*w] uint32, one texel per dword as c0 | c1 << 8 | c2 << 16, rows in the order given"""
    t = image.astype(np.uint32)
    return (t[..., 0] | (t[..., 1] << 8) | (t[..., 2] << 16)).reshape(-1)


class TexturedMeshTable(ShadedMeshTable):
    """A ``ShadedMeshTable`` with UV coordinates per vertex and one texture map per class, what ``inout.load_ply`` gives for a BOP model that names a
    texture file: everything that takes a MeshTable or a ShadedMeshTable takes it unchanged (``render_frames`` draws its vertex colours).
    ``colors_list``: as ShadedMeshTable; ``None`` (for the list or for one class) is 0.5 gray, as the reference draws a model without colours.
    ``textures[c]``: None, or the decoded image [h,w,3] as u8 or as floats in [0, 1] (rounded to u8 with rint), rows in FILE order (row 0 = the
    top) -- NOT flipped by the caller -- channels in any order: ``render_frames_bop`` writes the same order.  ``uv_list[c]``: [n_c,2], finite,
    required where a texture is given (v = 0 is the bottom row of the image); zeros elsewhere.  ``uvs`` [sum n_c,2] fp64, ``texels`` uint32 (one
    texel per dword), ``tex`` [C,3] int32 = (offset, h, w), h = 0 without a texture.  Wrong shapes, non-finite UVs, a texture side outside
    [1, 16384] or 2^31 texels and more raise ValueError."""

    TABLES = ShadedMeshTable.TABLES + ("uvs", "texels", "tex")

    def __init__(self, vertices_list, faces_list, colors_list=None, normals_list=None, uv_list=None, textures=None, device=None):
        C = len(vertices_list)
        for name, lst in (("colors_list", colors_list), ("uv_list", uv_list), ("textures", textures)):
            if lst is not None and len(lst) != C:
                raise ValueError(f"{name} needs one entry per class")
        nv = [np.asarray(v).reshape(-1, 3).shape[0] for v in vertices_list]
        colors_list = [None] * C if colors_list is None else list(colors_list)
        colors_list = [np.full((nv[c], 3), GRAY) if col is None else col for c, col in enumerate(colors_list)]
        super().__init__(vertices_list, faces_list, colors_list, normals_list)
        uvs, texels, tex, total = [], [], np.zeros((C, 3), dtype=np.int32), 0
        for c in range(C):
            n = int(self.nverts[c])
            image = None if textures is None else textures[c]
            uv = None if uv_list is None else uv_list[c]
            if uv is None:
                if image is not None:
                    raise ValueError(f"class {c} has a texture and no UV coordinates")
                uv = np.zeros((n, 2))
            uv = np.asarray(uv)
            if uv.shape != (n, 2) or not (np.issubdtype(uv.dtype, np.floating) or np.issubdtype(uv.dtype, np.integer)):
                raise ValueError(f"UV coordinates of class {c}: [{n}, 2] numbers, one pair per vertex")
            uv = uv.astype(np.float64)
            if not np.all(np.isfinite(uv)):
                raise ValueError(f"UV coordinates of class {c}: finite")
            uvs.append(uv)
            if image is None:
                continue
            image = np.asarray(image)
            if image.ndim != 3 or image.shape[2] != 3:
                raise ValueError(f"texture of class {c}: [h, w, 3]")
            h, w = image.shape[:2]
            if not (1 <= h <= TEX_MAX_SIDE and 1 <= w <= TEX_MAX_SIDE):
                raise ValueError(f"texture of class {c}: sides within [1, {TEX_MAX_SIDE}]")
            if np.issubdtype(image.dtype, np.floating):
                if not np.all(np.isfinite(image)) or image.min() < 0.0 or image.max() > 1.0:
                    raise ValueError(f"texture of class {c}: floats in [0, 1]")
                image = np.rint(255.0 * image.astype(np.float64)).astype(np.uint8)
            elif image.dtype != np.uint8:
                raise ValueError(f"texture of class {c}: u8 or floats in [0, 1]")
            tex[c] = (total, h, w)
            total += h * w
            if total >= 2 ** 31:
                raise ValueError("the texel table is indexed with int32 offsets")
            texels.append(pack_texels(image))
        self.uvs = np.ascontiguousarray(np.concatenate(uvs, axis=0))
        self.texels = np.ascontiguousarray(np.concatenate(texels)) if texels else np.zeros(0, dtype=np.uint32)
        self.tex = tex
        if device is not None:
            self.on(device)


def _texture_tables(table, dev):
    """(uvs, texels, tex on the device, tex on the host, n_texels) of a table; a plain ShadedMeshTable counts as untextured everywhere: zero UVs
    and an all-zero ``tex``, kept with the table's device copies"""
    if isinstance(table, TexturedMeshTable):
        tb = table.on(dev)
        return tb["uvs"], tb["texels"], tb["tex"], table.tex, int(table.texels.size)
    table.on(dev)
    cache = table.__dict__["_dev"].setdefault("untextured/" + str(dev), {})
    if not cache:
        cache.update(uvs=torch.zeros(int(table.verts.shape[0]), 2, dtype=torch.float64, device=dev),
                     tex=torch.zeros(table.num_classes, 3, dtype=torch.int32, device=dev), tex_host=np.zeros((table.num_classes, 3), dtype=np.int32))
    return cache["uvs"], None, cache["tex"], cache["tex_host"], 0


def render_frames_bop(table, labels, R, t, K, H, W, frame, num_frames=None, light=(0.0, 0.0, 0.0), ambient=AMBIENT, shading="phong",
                      filter="nearest", background=None, want_face=False, want_normals=False, near=render.NEAR, far=render.FAR):
    """Frames of N posed instances with the light model of the reference's BOP renderer (``lib/pysixd/renderer_py.py``, ``mode="rgb"``): the
    arguments, the visibility pass and the returned ``Frames`` of ``render_frames``, with another shading rule.  A class of a
    ``TexturedMeshTable`` that has a texture takes its base colour from the texture at the interpolated UV coordinates, every other class (and
    every class of a plain ``ShadedMeshTable``) from its vertex colours.  ``ambient``: a number or [F], finite and >= 0 (the reference's default
    0.5); ``light`` [3] or [F,3], camera coordinates in metres (default: the camera origin).  The pixel is ``round(255 min(1, ambient + max(N.L, 0))
    colour)``, half to even, without a specular term.  ``shading``: "phong" (interpolated vertex normals) or "flat" (the face normal, turned
    towards the camera).  ``filter``: "nearest" (the default) or "bilinear", both with clamp-to-edge and without mipmaps -- which of the two the
    reference's GL texture uses could not be established, so both exist.  ``Frames.normals`` reports the normal that was used."""
    if not isinstance(table, ShadedMeshTable):
        raise ValueError("render_frames_bop needs a ShadedMeshTable or a TexturedMeshTable")
    if shading not in SHADINGS or filter not in FILTERS:
        raise ValueError(f"shading: one of {sorted(SHADINGS)}; filter: one of {sorted(FILTERS)}")

    def weights(F):
        a = ambient.detach().cpu().numpy() if isinstance(ambient, torch.Tensor) else np.asarray(ambient)
        try:
            a = a.astype(np.float64)
        except (TypeError, ValueError):
            raise ValueError("ambient: a number or [F] numbers") from None
        if a.shape == ():
            a = np.broadcast_to(a, (F,))
        if a.shape != (F,) or not np.all(np.isfinite(a)) or (a.size and a.min() < 0.0):
            raise ValueError(f"ambient: a number or [{F}], finite and not negative")
        return np.ascontiguousarray(a)

    def launch(dev, vis, mesh, inst, maps):
        uvs, texels, tex, tex_host, n_texels = _texture_tables(table, dev)
        p = cabi.ptr
        cabi.check(cabi.load().gdrn_shade_frames_tex(vis, *mesh, p(uvs), p(texels), p(tex), tex_host.ctypes.data, n_texels, *inst, SHADINGS[shading],
                                                     FILTERS[filter], *maps), "shade_frames_tex")

    return _render(table, labels, R, t, K, H, W, frame, num_frames, light, weights, background, want_face, want_normals, near, far, launch)


def random_lights(F, rng, phong=PHONG):
    """(light [F,3], phong [F,3]) fp64 host arrays drawn from ``rng`` (a ``numpy.random.Generator``) with the distributions of
    ``render_many(random_light=True)`` (meshrenderer_phong.py:227-231): the position 1000 U(0,1)^3 mm in GL eye space, converted to camera
    coordinates in metres; each weight its ``phong`` value + 0.1 U(-1, 1), clipped at 0.  The distributions, not the reference's draws."""
    F = int(F)
    base = np.asarray(phong, dtype=np.float64).reshape(3)
    light = from_gl_eye_mm(1000.0 * rng.random((F, 3)))
    weights = np.maximum(base[None] + 0.1 * (2.0 * rng.random((F, 3)) - 1.0), 0.0)
    return light, weights
